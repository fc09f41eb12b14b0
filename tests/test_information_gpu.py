"""GPU: ``sdfr_render_information`` (through ``sdfest_amd.render_information``) against the float64 twin built from the
oracle's per-pixel derivative images (tests/information_twin.py), on the committed golden scenes.

Set-up of every test: the estimate image is the HIP forward at the scene's pose and the target the HIP forward at the
perturbed pose (information_twin.perturbed_pose); the same fp32 images go to the kernel and to the oracle -- the same
hit points for everybody, as in test_render_gpu.test_backward_matches_oracle_and_golden.

The bound: every entry of the Gram matrix within REL * sum_pixels |f_i f_j| of the twin's, REL = 1e-4 being the
project's tolerance for fp32 gradients (test_render_gpu.REL), applied the way its ``pose_l1`` applies it -- relative
to the sum of magnitudes, which is what fp32 per-pixel rounding and summation errors scale with."""
import functools

import numpy as np
import pytest
import torch

import information_twin as twin
from helpers import load_render_case, render_cases
from test_render_gpu import REL, dev, hip_backward, hip_forward

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import sdfest_amd.differentiable_renderer as r
    assert torch.cuda.is_available()
    return r


def camera_of(c):
    from sdfest_amd import Camera
    return Camera(c["W"], c["H"], c["fx"], c["fy"], c["cx"], c["cy"], pixel_center=0.5)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(case, depth, target, features): the two HIP forwards and the twin's (H,W,10) feature image, made once."""
    import sdfest_amd.differentiable_renderer as r
    c = load_render_case(name)
    cam = (c["W"], c["H"], c["cx"], c["cy"], c["fx"], c["fy"])
    depth = hip_forward(r, c["sdf"], c["p"], c["q"], [c["inv_scale"]], *cam, c["thr"])[0]
    tp, tq, ts = twin.perturbed_pose(c["p"], c["q"], c["inv_scale"])
    target = hip_forward(r, c["sdf"], tp, tq, [ts], *cam, c["thr"])[0]
    f = twin.features(depth, target, c["sdf"], c["p"], c["q"], c["inv_scale"], *cam[2:])
    return c, depth, target, f


def information(c, depth, target, thr=0.0, sdf=None, workspace=None):
    """render_information on numpy inputs of one or several views that share the camera of `c`."""
    from sdfest_amd import render_information
    p = np.asarray(c["p"], np.float32).reshape(-1, 3)
    q = np.asarray(c["q"], np.float32).reshape(-1, 4)
    s = np.asarray(c["inv_scale"], np.float32).reshape(-1)
    g = render_information(dev(np.asarray(depth).reshape(len(p), c["H"], c["W"])),
                           dev(np.asarray(target).reshape(len(p), c["H"], c["W"])), dev(c["sdf"] if sdf is None else sdf),
                           dev(p), dev(q), dev(s), camera_of(c), thr, workspace=workspace)
    assert g.dtype == torch.float64 and g.shape == (len(p), 10, 10) and g.is_cuda
    return g


def check_bound(g, ref, yard, name):
    err = np.abs(g - ref)
    print(f"{name}: worst entry at {np.max(err / np.maximum(yard, 1e-300)):.3e} of sum |f_i f_j| (bound {REL:.0e})")
    assert np.all(err <= REL * yard + 1e-300), (name, np.max(err / np.maximum(yard, 1e-300)))


@pytest.mark.parametrize("name", render_cases())
def test_matches_the_float64_twin(name):
    c, depth, target, f = scene(name)
    g = information(c, depth, target)[0].cpu().numpy()
    inc = twin.included(depth, target)
    ref, yard = twin.gram(f, inc)
    print(f"{name}: {int(inc.sum())} included pixels")
    if name in ("g4_behind_32x24", "g4_offscreen_32x24"):
        assert not inc.any()
    if not inc.any():
        assert not g.any() and not np.signbit(g).any()      # an empty view: exactly zero
    else:
        check_bound(g, ref, yard, name)
        assert g[9, 9] == inc.sum()


@pytest.mark.parametrize("name", ["g1_sphere_32x24", "g4_parallel_slab_33x25", "g2_blobs_c1_160x120", "g4_behind_32x24"])
def test_count_symmetry_and_reproducibility_are_exact(name):
    from sdfest_amd import _lib
    c, depth, target, _ = scene(name)
    g = information(c, depth, target)
    assert g[0, 9, 9].item() == int(twin.included(depth, target).sum())     # numpy float32's inclusion set
    assert torch.equal(g, g.transpose(1, 2))
    assert torch.equal(g, information(c, depth, target))
    n = _lib.lib().sdfr_render_information_workspace_bytes(1, c["W"], c["H"])
    ws = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")            # every word a NaN, every flag set
    assert torch.equal(g, information(c, depth, target, workspace=ws))
    assert torch.equal(g, information(c, depth, target, workspace=ws))       # ... and what the call itself left there


def test_inlier_threshold_selects_numpy_float32s_pixels():
    c, depth, target, f = scene("g2_blobs_c1_160x120")
    overlap, inc = twin.included(depth, target), twin.included(depth, target, 0.03)
    assert 0 < inc.sum() < overlap.sum(), (inc.sum(), overlap.sum())        # the threshold does cut into the overlap
    g = information(c, depth, target, thr=0.03)[0].cpu().numpy()
    assert g[9, 9] == inc.sum()
    ref, yard = twin.gram(f, inc)
    check_bound(g, ref, yard, "g2 at 0.03")
    assert np.array_equal(g, g.T)


def test_a_view_does_not_depend_on_its_batch():
    # three poses over one shared grid
    names = ("g3_pose0_64x48", "g3_pose2_64x48", "g4_behind_32x24")
    c0 = scene(names[0])[0]
    cam = (c0["W"], c0["H"], c0["cx"], c0["cy"], c0["fx"], c0["fy"])
    import sdfest_amd.differentiable_renderer as r
    poses = [load_render_case(n) for n in names]
    P = np.stack([np.asarray(c["p"], np.float64) for c in poses])
    Q = np.stack([np.asarray(c["q"], np.float64) for c in poses])
    S = np.array([c["inv_scale"] for c in poses])
    pert = [twin.perturbed_pose(p, q, s) for p, q, s in zip(P, Q, S)]
    depth = hip_forward(r, c0["sdf"], P, Q, S, *cam, c0["thr"])
    target = hip_forward(r, c0["sdf"], np.stack([t[0] for t in pert]), np.stack([t[1] for t in pert]),
                         np.array([t[2] for t in pert]), *cam, c0["thr"])
    batch = dict(c0, p=P, q=Q, inv_scale=S)
    g = information(batch, depth, target)
    assert g[0, 9, 9] > 0 and g[1, 9, 9] > 0 and not g[2].any()
    for b in range(3):
        one = dict(c0, p=P[b], q=Q[b], inv_scale=S[b])
        assert torch.equal(g[b], information(one, depth[b], target[b])[0]), b
    # per-view grids: a sphere and the blobs
    from oracle import blobs_sdf, sphere_sdf
    vols = np.stack([sphere_sdf(0.5), blobs_sdf(0), sphere_sdf(0.5)]).astype(np.float32)
    depth = np.stack([hip_forward(r, vols[b], P[b], Q[b], S[b:b + 1], *cam, c0["thr"])[0] for b in range(3)])
    target = np.stack([hip_forward(r, vols[b], pert[b][0], pert[b][1], [pert[b][2]], *cam, c0["thr"])[0] for b in range(3)])
    g = information(batch, depth, target, sdf=vols)
    assert g[0, 9, 9] > 0 and g[1, 9, 9] > 0
    for b in range(3):
        one = dict(c0, p=P[b], q=Q[b], inv_scale=S[b])
        assert torch.equal(g[b], information(one, depth[b], target[b], sdf=vols[b])[0]), b


@pytest.mark.parametrize("name", ["g3_pose1_64x48", "g2_blobs_c1_160x120", "g4_partly_out_48x32"])
def test_gradient_column_agrees_with_the_backward(R, name):
    """J^T r is what sdfr_render_backward returns for the upstream image r on the included pixels."""
    c, depth, target, f = scene(name)
    inc = twin.included(depth, target)
    g = information(c, depth, target)[0].cpu().numpy()
    up = np.where(inc, depth - target, np.float32(0)).astype(np.float32)
    cam = (c["W"], c["H"], c["cx"], c["cy"], c["fx"], c["fy"])
    _, g_pos, g_quat, g_isc = hip_backward(R, up, depth, c["sdf"], c["p"], c["q"], [c["inv_scale"]], *cam)
    pose = np.concatenate([g_pos[0], g_quat[0], g_isc]).astype(np.float64)
    _, yard = twin.gram(f, inc)
    assert inc.any() and np.all(np.abs(g[:8, 8] - pose) <= REL * yard[:8, 8]), (g[:8, 8], pose)
