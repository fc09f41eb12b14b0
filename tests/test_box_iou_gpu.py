"""GPU: sdfr_box_iou (csrc/boxes.hip) through sdfest_amd.box_iou -- scipy's volumes of 300 general-position pairs
(tests/golden/box_iou.npz), closed forms in the degenerate positions, the numpy twin (tests/box_iou_twin.py) for the
symmetry maximum, and the contract: an entry depends on its own two boxes alone, invalid boxes give NaN, the same bits
on every call.  The yardstick everywhere: 1e-12 L^3 for a volume, L = |e_a| + |e_b| + |c_b - c_a|."""
import numpy as np
import pytest
import torch

import box_iou_twin as twin
from helpers import GOLDEN

pytestmark = pytest.mark.gpu


def iou(a_rows, b_rows, **kw):
    from sdfest_amd import box_iou
    a, b = np.asarray(a_rows, np.float64).reshape(-1, 10), np.asarray(b_rows, np.float64).reshape(-1, 10)
    out = box_iou(a[:, :3], a[:, 3:7], a[:, 7:], b[:, :3], b[:, 3:7], b[:, 7:], **kw)
    return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    g = np.load(f"{GOLDEN}/box_iou.npz")
    a, b = g["boxes_a"], g["boxes_b"]
    L = (np.linalg.norm(a[:, 7:], axis=1) + np.linalg.norm(b[:, 7:], axis=1) + np.linalg.norm(b[:, :3] - a[:, :3], axis=1))
    return a, b, g["volume"], L


@pytest.fixture(scope="module")
def paired(golden):
    a, b, _, _ = golden
    return iou(a, b, paired=True, return_intersection=True)


def test_golden_pairs_volume_and_iou(golden, paired):
    a, b, volume, L = golden
    got_iou, got_volume = paired
    assert got_iou.shape == got_volume.shape == (300,) and got_iou.dtype == np.float64
    bound = 1e-12 * L ** 3
    union = a[:, 7:].prod(1) + b[:, 7:].prod(1) - volume
    print(f"worst |V - V_gold| / L^3 = {np.max(np.abs(got_volume - volume) / L ** 3):.3e}, "
          f"worst IoU error over its bound = {np.max(np.abs(got_iou - volume / union) / (2 * bound / union)):.3e}")
    assert np.all(np.abs(got_volume - volume) <= bound)
    assert np.all(np.abs(got_iou - volume / union) <= 2 * bound / union)
    assert np.all(got_volume >= 0) and np.all(got_volume[volume == 0] == 0)


@pytest.mark.parametrize("name, a, b, kind, expected", twin.CLOSED_FORMS, ids=[c[0] for c in twin.CLOSED_FORMS])
def test_closed_forms(name, a, b, kind, expected):
    got_iou, got_volume = iou(twin.rows([a]), twin.rows([b]), return_intersection=True)
    assert got_iou.shape == (1, 1)
    got = got_iou[0, 0] if kind == "iou" else got_volume[0, 0]
    print(f"{name}: {got!r} (expected {expected!r})")
    assert abs(got - expected) <= twin.closed_form_bound(a, b, kind, expected)
    assert got_volume[0, 0] >= 0.0 and got_iou[0, 0] <= 1.0


def test_disjoint_boxes_give_exactly_zero():
    a, b = twin.FAR_APART
    got_iou, got_volume = iou(twin.rows([a]), twin.rows([b]), return_intersection=True)
    assert got_iou[0, 0] == 0.0 and got_volume[0, 0] == 0.0
    # apart, but with overlapping bounding spheres: two thin slabs side by side
    slab = (np.zeros(3), twin.GENERIC_Q, np.array([1.0, 1.0, 0.01]))
    shift = twin.rotation(twin.GENERIC_Q) @ np.array([0.0, 0.0, 0.1])
    got_iou, got_volume = iou(twin.rows([slab]), twin.rows([(shift, twin.GENERIC_Q, slab[2])]), return_intersection=True)
    assert got_iou[0, 0] == 0.0 and got_volume[0, 0] == 0.0


def test_matrix_entries_are_bitwise_the_paired_results(golden):
    a, b, _, _ = golden
    m_iou, m_vol = iou(a[:3], b[10:15], return_intersection=True)
    assert m_iou.shape == (3, 5)
    for i in range(3):
        for j in range(5):
            p_iou, p_vol = iou(a[i], b[10 + j], paired=True, return_intersection=True)       # K = 1
            assert p_iou[0].tobytes() == m_iou[i, j].tobytes() and p_vol[0].tobytes() == m_vol[i, j].tobytes()
    # the same pairs inside a batch that crosses a wave (K = 65), at other places
    ia, ib = np.arange(65) % 3, 10 + np.arange(65) % 5
    p_iou, p_vol = iou(a[ia], b[ib], paired=True, return_intersection=True)
    assert p_iou.shape == (65,)
    assert p_iou.tobytes() == m_iou[ia, ib - 10].tobytes() and p_vol.tobytes() == m_vol[ia, ib - 10].tobytes()


def test_swapping_the_boxes(golden, paired):
    a, b, _, L = golden
    s_iou, s_vol = iou(b, a, paired=True, return_intersection=True)
    bound = 1e-12 * L ** 3
    union = a[:, 7:].prod(1) + b[:, 7:].prod(1) - paired[1]
    assert np.all(np.abs(s_vol - paired[1]) <= bound) and np.all(np.abs(s_iou - paired[0]) <= 2 * bound / union)


def test_symmetry(golden, paired):
    a45, b45 = twin.CUBES_45
    got = iou(twin.rows([a45]), twin.rows([b45]), rotational_symmetry_axis=2, symmetry_steps=8)
    assert abs(got[0, 0] - 1.0) <= twin.closed_form_bound(a45, b45, "iou", 1.0) and got[0, 0] <= 1.0
    # about another axis the turn stays
    other = iou(twin.rows([a45]), twin.rows([b45]), rotational_symmetry_axis=0, symmetry_steps=8)
    plain = iou(twin.rows([a45]), twin.rows([b45]))
    assert plain[0, 0] <= other[0, 0] < 0.9  # step 0 is among the candidates; no turn about x undoes one about z
    # one step is no symmetry, bitwise
    a, b, _, L = golden
    one = iou(a, b, paired=True, rotational_symmetry_axis=1, symmetry_steps=1, return_intersection=True)
    assert one[0].tobytes() == paired[0].tobytes() and one[1].tobytes() == paired[1].tobytes()
    # generic pairs against the twin's maximum: 20 steps (one group of lanes per pair) and 70 (more steps than lanes)
    for axis, steps, k in ((0, 20, 3), (1, 20, 3), (2, 20, 3), (2, 70, 4), (1, 3, 5)):
        got_iou, got_vol = iou(a[k], b[k], paired=True, rotational_symmetry_axis=axis, symmetry_steps=steps,
                               return_intersection=True)
        V, I = twin.box_intersection((a[k, :3], a[k, 3:7], a[k, 7:]), (b[k, :3], b[k, 3:7], b[k, 7:]), axis, steps)
        bound = 1e-12 * L[k] ** 3
        union = a[k, 7:].prod() + b[k, 7:].prod() - V
        print(f"axis {axis}, {steps} steps: V {got_vol[0]!r} (twin {V!r}), IoU {got_iou[0]!r}")
        assert abs(got_vol[0] - V) <= bound and abs(got_iou[0] - I) <= 2 * bound / union
        assert got_vol[0] >= paired[1][k]
    # in a batch (three pairs per workgroup at 20 steps), entry by entry the same bits as alone
    batch = iou(a[:7], b[:7], paired=True, rotational_symmetry_axis=2, symmetry_steps=20)
    for k in range(7):
        alone = iou(a[k], b[k], paired=True, rotational_symmetry_axis=2, symmetry_steps=20)
        assert alone[0].tobytes() == batch[k].tobytes()


def test_invalid_boxes_give_nan_and_leave_the_others(golden):
    a, b, _, _ = golden
    a, b = a[:4].copy(), b[:5].copy()
    clean = iou(a, b, return_intersection=True)
    a[1, 0] = np.inf            # a non-finite entry
    b[2, 8] = 0.0               # a non-positive extent
    b[4, 3:7] = 0.0             # a zero quaternion
    a[3, 9] = np.nan
    got = iou(a, b, return_intersection=True)
    bad = np.zeros((4, 5), dtype=bool)
    bad[[1, 3], :] = True
    bad[:, [2, 4]] = True
    for g, c in zip(got, clean):
        assert np.isnan(g[bad]).all()
        assert g[~bad].tobytes() == c[~bad].tobytes()
    negative = b[:1].copy()
    negative[0, 7] = -0.1
    assert np.isnan(iou(a[:1], negative)).all()


def test_empty_batches_and_repeatability(golden, paired):
    a, b, _, _ = golden
    assert iou(a[:0], b[:3]).shape == (0, 3) and iou(a[:2], b[:0]).shape == (2, 0)
    assert iou(a[:0], b[:0], paired=True).shape == (0,)
    again = iou(a, b, paired=True, return_intersection=True)
    assert again[0].tobytes() == paired[0].tobytes() and again[1].tobytes() == paired[1].tobytes()
    # float32 inputs and device tensors are taken as they are
    from sdfest_amd import box_iou
    t = lambda x: torch.tensor(x, dtype=torch.float32, device="cuda")
    f32 = box_iou(t(a[:3, :3]), t(a[:3, 3:7]), t(a[:3, 7:]), t(b[:3, :3]), t(b[:3, 3:7]), t(b[:3, 7:]), paired=True)
    assert f32.dtype == torch.float64 and f32.is_cuda
    assert np.allclose(f32.cpu().numpy(), paired[0][:3], atol=1e-5)


def test_correct_thresh_flips_across_the_iou():
    """unit cubes half a side apart: IoU 1/3"""
    from sdfest_amd.metrics import correct_thresh, iou_3d
    (ca, qa, ea), (cb, qb, eb) = twin.CLOSED_FORMS[1][1], twin.CLOSED_FORMS[1][2]
    assert abs(iou_3d(ca, qa, ea, cb, qb, eb) - 1.0 / 3.0) <= 1e-12
    call = lambda t, **kw: correct_thresh(ca, cb, qa, qb, extent_gt=ea, extent_prediction=eb, iou_3d_threshold=t, **kw)
    assert call(1.0 / 3.0 - 1e-9) == 1 and call(1.0 / 3.0 + 1e-9) == 0
    assert call(0.5) == 0 and call(0.25) == 1
    assert call(0.25, position_threshold=0.4) == 0 and call(0.25, position_threshold=0.6, degree_threshold=1.0) == 1
    # the symmetry axis is passed through: unit cubes 36 degrees apart about z, two of the 20 steps (IoU 0.716 as they
    # are: the octagon's area is 2 / (1 + sin + cos))
    (ca, qa, ea), (cb, qb, eb) = twin.CUBES_45
    qb = twin._quat_z(36.0)
    turned = lambda **kw: correct_thresh(ca, cb, qa, torch.tensor(qb), extent_gt=ea, extent_prediction=torch.tensor(eb),
                                         iou_3d_threshold=0.9, **kw)
    assert turned() == 0 and turned(rotational_symmetry_axis=2) == 1
