"""CPU: the numpy twin of the box intersection (tests/box_iou_twin.py) against scipy's volumes of 300 general-position
pairs (tests/golden/box_iou.npz, tools/make_box_iou_goldens.py) and against closed forms in the degenerate positions;
Mesh.oriented_box on a CPU mesh; the Python shape errors and the C ABI's argument errors, which come before any GPU
call."""
import ctypes

import numpy as np
import pytest
import torch

import box_iou_twin as twin
from helpers import GOLDEN


def test_twin_matches_scipy_on_general_position_pairs():
    """|V - V_gold| <= 1e-12 L^3: each product of the sum is bounded by L^3 and a few hundred float64 roundings give
    about 1e-13 of it; a wrong clip is off by a share of the volume."""
    g = np.load(f"{GOLDEN}/box_iou.npz")
    assert g["boxes_a"].shape == g["boxes_b"].shape == (300, 10) and (g["volume"] > 0).sum() >= 150
    worst = 0.0
    for a, b, v in zip(g["boxes_a"], g["boxes_b"], g["volume"]):
        V, iou = twin.box_intersection((a[:3], a[3:7], a[7:]), (b[:3], b[3:7], b[7:]))
        L = twin.length_scale(a[:3], a[7:], b[:3], b[7:])
        worst = max(worst, abs(V - v) / L ** 3)
        assert abs(V - v) <= 1e-12 * L ** 3
        assert iou == V / (np.prod(a[7:]) + np.prod(b[7:]) - V)
    print(f"worst |V - V_gold| / L^3 = {worst:.3e}")


@pytest.mark.parametrize("name, a, b, kind, expected", twin.CLOSED_FORMS, ids=[c[0] for c in twin.CLOSED_FORMS])
def test_twin_closed_forms(name, a, b, kind, expected):
    V, iou = twin.box_intersection(a, b)
    got = iou if kind == "iou" else V
    print(f"{name}: {got!r} (expected {expected!r})")
    assert abs(got - expected) <= twin.closed_form_bound(a, b, kind, expected)
    assert V >= 0.0


def test_twin_disjoint_is_exactly_zero_and_symmetry_finds_the_turn():
    assert twin.box_intersection(*twin.FAR_APART) == (0.0, 0.0)
    a, b = twin.CUBES_45
    V, iou = twin.box_intersection(a, b, symmetry_axis=2, symmetry_steps=8)
    assert abs(iou - 1.0) <= twin.closed_form_bound(a, b, "iou", 1.0)
    assert twin.box_intersection(a, b, symmetry_axis=2, symmetry_steps=1) == twin.box_intersection(a, b)


def test_oriented_box_of_a_posed_cpu_mesh():
    from sdfest_amd import Mesh
    half = np.array([0.05, 0.035, 0.08])
    offset = np.array([0.01, -0.02, 0.03])     # the box's middle is not the mesh's origin
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * half + offset
    q = twin.GENERIC_Q / np.linalg.norm(twin.GENERIC_Q)
    mesh = Mesh(torch.tensor(v, dtype=torch.float32), torch.zeros((0, 3), dtype=torch.int32), scale=2.0, rel_scale=True,
                position=[0.3, -0.1, 0.7], orientation=q)
    lo, hi = mesh.bounding_box()
    assert np.allclose(lo.numpy(), 2 * (offset - half), atol=1e-7) and np.allclose(hi.numpy(), 2 * (offset + half), atol=1e-7)
    center, orientation, extents = mesh.oriented_box()
    assert center.shape == (3,) and orientation.shape == (4,) and extents.shape == (3,) and not center.is_cuda
    c, _, e = twin.tight_box(2 * v, [0.3, -0.1, 0.7], q)
    assert np.allclose(center.numpy(), c, atol=1e-6) and np.allclose(extents.numpy(), e, atol=1e-6)
    assert np.allclose(orientation.numpy(), q, atol=1e-7)
    assert center.dtype == orientation.dtype == extents.dtype == torch.float64
    # a pose given to the call keeps its precision: the box of exactly that float64 pose
    p64, q64 = torch.tensor([0.3, -0.1, 0.7], dtype=torch.float64), torch.tensor(q)
    center, orientation, extents = mesh.oriented_box(p64, q64)
    c, _, e = twin.tight_box(mesh.scaled_vertices().double().numpy(), p64.numpy(), q)
    assert torch.equal(orientation, q64) and np.allclose(center.numpy(), c, rtol=0, atol=1e-15)
    assert np.allclose(extents.numpy(), e, rtol=0, atol=1e-15)
    # every posed vertex lies in the box
    local = (mesh.transformed_vertices().double().numpy() - center.double().numpy()) @ twin.rotation(q)
    assert np.all(np.abs(local) <= extents.double().numpy() / 2 + 1e-6)
    with pytest.raises(ValueError):
        Mesh(torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int32)).oriented_box()


def test_python_shape_errors_before_the_gpu():
    from sdfest_amd import box_iou, sdf_bounds
    c, q, e = np.zeros((2, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (2, 1)), np.ones((2, 3))
    with pytest.raises(ValueError):
        box_iou(np.zeros((2, 4)), q, e, c, q, e)
    with pytest.raises(ValueError):
        box_iou(c, q[:, :3], e, c, q, e)
    with pytest.raises(ValueError):
        box_iou(c, q, e, c, q, np.ones((3, 3)))
    with pytest.raises(ValueError):
        box_iou(c, q, e, c[:1], q[:1], e[:1], paired=True)
    with pytest.raises(ValueError):
        box_iou(c, q, e, c, q, e, rotational_symmetry_axis=3)
    with pytest.raises(ValueError):
        box_iou(c, q, e, c, q, e, rotational_symmetry_axis=1, symmetry_steps=0)
    with pytest.raises(ValueError):
        sdf_bounds(torch.zeros((4, 4, 5)), 0.0)
    with pytest.raises(ValueError):
        sdf_bounds(torch.zeros((4, 4)), 0.0)
    with pytest.raises(TypeError):
        sdf_bounds(torch.zeros((4, 4, 4)), 0.0)          # not on the device


def test_correct_thresh_without_extents_still_raises():
    from sdfest_amd.metrics import correct_thresh
    for kw in ({}, {"extent_gt": np.ones(3)}, {"extent_prediction": np.ones(3)}):
        with pytest.raises(NotImplementedError, match="extent"):
            correct_thresh(np.zeros(3), np.zeros(3), [0, 0, 0, 1], [0, 0, 0, 1], iou_3d_threshold=0.5, **kw)


def test_c_abi_argument_errors_without_gpu():
    from sdfest_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert _lib.SIGNATURES["sdfr_box_iou"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                              ctypes.c_void_p])
    assert (_lib.ABI["SDFR_BOX_IOU_MATRIX"], _lib.ABI["SDFR_BOX_IOU_PAIRED"]) == (0, 1)
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)        # a non-NULL pointer that is never dereferenced
    odd = ctypes.c_void_p(q.value + 4)
    err = lambda: L.sdfr_last_error()
    invalid = _lib.ABI["SDFR_E_INVALID"]
    # sdfr_sdf_bounds
    assert L.sdfr_sdf_bounds(q, 1, 1, 0, 0.0, q, q, 0, None) == invalid and b"R=1" in err()
    assert L.sdfr_sdf_bounds(q, 1, 257, 0, 0.0, q, q, 0, None) == invalid
    assert L.sdfr_sdf_bounds(q, -1, 8, 0, 0.0, q, q, 0, None) == invalid and b"N=-1" in err()
    assert L.sdfr_sdf_bounds(q, 65536, 8, 0, 0.0, q, q, 0, None) == invalid
    assert L.sdfr_sdf_bounds(q, 1, 8, 2, 0.0, q, q, 0, None) == invalid and b"complete" in err()
    assert L.sdfr_sdf_bounds(q, 1, 8, 0, float("nan"), q, q, 0, None) == invalid and b"level" in err()
    assert L.sdfr_sdf_bounds(None, 1, 8, 0, 0.0, q, q, 0, None) == invalid and b"NULL" in err()
    assert L.sdfr_sdf_bounds(q, 1, 8, 0, 0.0, q, None, 0, None) == invalid
    assert L.sdfr_sdf_bounds(None, 0, 8, 0, 0.0, None, None, 0, None) == 0        # nothing to do
    # sdfr_box_iou
    assert L.sdfr_box_iou(q, -1, q, 1, 0, -1, 1, q, None, 0, None) == invalid
    assert L.sdfr_box_iou(q, 2, q, 3, 1, -1, 1, q, None, 0, None) == invalid and b"N == M" in err()
    assert L.sdfr_box_iou(q, 2, q, 2, 2, -1, 1, q, None, 0, None) == invalid and b"mode" in err()
    assert L.sdfr_box_iou(q, 2, q, 2, 0, 3, 1, q, None, 0, None) == invalid and b"symmetry_axis" in err()
    assert L.sdfr_box_iou(q, 2, q, 2, 0, 1, 0, q, None, 0, None) == invalid and b"symmetry_steps" in err()
    assert L.sdfr_box_iou(None, 2, q, 2, 0, -1, 1, q, None, 0, None) == invalid and b"NULL" in err()
    assert L.sdfr_box_iou(q, 2, q, 2, 0, -1, 1, None, None, 0, None) == invalid
    assert L.sdfr_box_iou(q, 2, q, 2, 0, -1, 1, odd, None, 0, None) == invalid and b"aligned" in err()
    assert L.sdfr_box_iou(None, 0, q, 2, 0, -1, 1, None, None, 0, None) == 0      # nothing to do
    assert L.sdfr_box_iou(q, 2, None, 0, 0, 2, 20, None, None, 0, None) == 0
