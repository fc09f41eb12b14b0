"""GPU: ``sdfr_render_information_shape`` (through ``sdfest_amd.render_information(jacobian=)``) against the float64
twin (tests/shape_information_twin.py: the oracle's pose derivative images, and the oracle's d depth / d SDF of every
included pixel contracted with the tangent volumes), and ``sdfr_sdf_std`` against a float64 einsum.

Set-up as tests/test_information_gpu.py: the estimate is the HIP forward at the scene's pose, the target the HIP forward
at the perturbed pose, the same fp32 images for the kernel and the oracle.  The tangent volumes are seeded smooth fields
(``shape_information_twin.tangent_fields``), T of them with T in {1, 8, 22}: the kernel test does not depend on the
decoder.  The bound is that file's: every entry within 1e-4 x sum_pixels |f_i f_j| of the twin's."""
import functools

import numpy as np
import pytest
import torch

import information_twin as twin
import shape_information_twin as st
from test_information_gpu import camera_of, check_bound, information, scene
from test_render_gpu import REL, dev, hip_backward

pytestmark = pytest.mark.gpu

SCENES = ("g1_sphere_32x24", "g3_pose1_64x48", "g4_parallel_slab_33x25")
EMPTY = "g4_offscreen_32x24"
TS = (1, 8, 22)


@functools.lru_cache(maxsize=None)
def latent_image(name):
    """(H,W,22) float64: the twin's latent features of all 22 fields on the scene's included pixels, made once"""
    c, depth, target, _ = scene(name)
    return st.latent_features(depth, c["sdf"], c["p"], c["q"], c["inv_scale"], c["cx"], c["cy"], c["fx"], c["fy"],
                              twin.included(depth, target), st.tangent_fields())


@functools.lru_cache(maxsize=None)
def jac_of(T):
    return dev(st.jac_buffer(st.tangent_fields(), T))


def shape_information(c, depth, target, T, thr=0.0, sdf=None, jac=None, workspace=None):
    """render_information(jacobian=) on numpy inputs of one or several views that share the camera of `c`"""
    from sdfest_amd import render_information
    p = np.asarray(c["p"], np.float32).reshape(-1, 3)
    q = np.asarray(c["q"], np.float32).reshape(-1, 4)
    s = np.asarray(c["inv_scale"], np.float32).reshape(-1)
    g = render_information(dev(np.asarray(depth).reshape(len(p), c["H"], c["W"])),
                           dev(np.asarray(target).reshape(len(p), c["H"], c["W"])), dev(c["sdf"] if sdf is None else sdf),
                           dev(p), dev(q), dev(s), camera_of(c), thr, workspace=workspace,
                           jacobian=jac_of(T) if jac is None else jac, tangents=T)
    assert g.dtype == torch.float64 and g.shape == (len(p), 10 + T, 10 + T) and g.is_cuda
    return g


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", SCENES)
def test_matches_the_float64_twin_and_the_pose_call(name, T):
    c, depth, target, f10 = scene(name)
    inc = twin.included(depth, target)
    assert inc.any()
    g = shape_information(c, depth, target, T)[0].cpu().numpy()
    ref, yard = twin.gram(st.joint_features(f10, latent_image(name), T), inc)
    check_bound(g, ref, yard, f"{name} T={T}")
    assert g[9 + T, 9 + T] == inc.sum()
    # the pose block, J^T r and sum r^2 of sdfr_render_information on the same inputs; the count exactly
    g10 = information(c, depth, target)[0].cpu().numpy()
    pick = np.r_[0:8, 8 + T, 9 + T]
    sub, ysub = g[np.ix_(pick, pick)], yard[np.ix_(pick, pick)]
    print(f"{name} T={T}: against the pose call {np.max(np.abs(sub - g10) / np.maximum(ysub, 1e-300)):.3e} of sum |f_i f_j|")
    assert np.all(np.abs(sub - g10) <= REL * ysub) and sub[9, 9] == g10[9, 9]


@pytest.mark.parametrize("T", TS)
def test_symmetry_reproducibility_and_the_empty_view_are_exact(T):
    from sdfest_amd import _lib
    for name in ("g3_pose1_64x48", "g4_parallel_slab_33x25", EMPTY):
        c, depth, target, _ = scene(name)
        g = shape_information(c, depth, target, T)
        assert torch.equal(g, g.transpose(1, 2))
        assert torch.equal(g, shape_information(c, depth, target, T))
        n = _lib.lib().sdfr_render_information_shape_workspace_bytes(1, c["W"], c["H"], T)
        ws = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")            # every word a NaN, every flag set
        assert torch.equal(g, shape_information(c, depth, target, T, workspace=ws))
        assert torch.equal(g, shape_information(c, depth, target, T, workspace=ws))
        if name == EMPTY:
            assert not twin.included(depth, target).any()
            assert not g.any().item() and not torch.signbit(g).any().item()      # exactly zero
        else:
            # an all-zero Jacobian: exactly zero latent rows and columns, the rest unchanged
            z = shape_information(c, depth, target, T, jac=torch.zeros_like(jac_of(T)))[0]
            assert not z[8:8 + T, :].any().item() and not z[:, 8:8 + T].any().item()
            keep = [i for i in range(10 + T) if not 8 <= i < 8 + T]
            assert torch.equal(z[keep][:, keep], g[0][keep][:, keep])


@pytest.mark.parametrize("name", SCENES)
def test_inlier_threshold_selects_numpy_float32s_pixels(name):
    c, depth, target, f10 = scene(name)
    inc = twin.included(depth, target, 0.03)
    print(f"{name}: {int(inc.sum())} of {int(twin.included(depth, target).sum())} overlap pixels within 0.03")
    g = shape_information(c, depth, target, 8, thr=0.03)[0].cpu().numpy()
    assert g[17, 17] == inc.sum()
    if inc.any():
        ref, yard = twin.gram(st.joint_features(f10, latent_image(name), 8), inc)
        check_bound(g, ref, yard, f"{name} at 0.03")


def test_a_view_does_not_depend_on_its_batch():
    import sdfest_amd.differentiable_renderer as r
    from helpers import load_render_case
    from test_render_gpu import hip_forward
    T = 8
    names = ("g3_pose0_64x48", "g3_pose2_64x48", EMPTY)
    c0 = scene(names[0])[0]
    cam = (c0["W"], c0["H"], c0["cx"], c0["cy"], c0["fx"], c0["fy"])
    poses = [load_render_case(n) for n in names]
    P = np.stack([np.asarray(c["p"], np.float64) for c in poses])
    Q = np.stack([np.asarray(c["q"], np.float64) for c in poses])
    S = np.array([c["inv_scale"] for c in poses])
    pert = [twin.perturbed_pose(p, q, s) for p, q, s in zip(P, Q, S)]
    depth = hip_forward(r, c0["sdf"], P, Q, S, *cam, c0["thr"])
    target = hip_forward(r, c0["sdf"], np.stack([t[0] for t in pert]), np.stack([t[1] for t in pert]),
                         np.array([t[2] for t in pert]), *cam, c0["thr"])
    batch = dict(c0, p=P, q=Q, inv_scale=S)
    # a shared Jacobian
    g = shape_information(batch, depth, target, T)
    assert g[0, 17, 17] > 0 and g[1, 17, 17] > 0 and not g[2].any()
    for b in range(3):
        one = dict(c0, p=P[b], q=Q[b], inv_scale=S[b])
        assert torch.equal(g[b], shape_information(one, depth[b], target[b], T)[0]), b
    # a Jacobian per view (jac_view_stride): the fields in three different orders
    fields = st.tangent_fields()
    jacs = torch.stack([dev(st.jac_buffer(fields[order], T)) for order in (np.arange(8), np.arange(8)[::-1], np.arange(8, 16))])
    g = shape_information(batch, depth, target, T, jac=jacs)
    for b in range(3):
        one = dict(c0, p=P[b], q=Q[b], inv_scale=S[b])
        assert torch.equal(g[b], shape_information(one, depth[b], target[b], T, jac=jacs[b].contiguous())[0]), b
    # (view 0 reads the shared call's fields, view 1 the same fields in another order: the stride does select)
    shared = shape_information(batch, depth, target, T)
    assert torch.equal(g[0], shared[0]) and not torch.equal(g[1], shared[1])


@pytest.mark.parametrize("name", ["g3_pose1_64x48", "g4_parallel_slab_33x25"])
def test_latent_gradient_column_agrees_with_the_backward(name):
    """the latent part of J^T r is sdfr_render_backward's g_sdf for the upstream image r on the included pixels,
    contracted with the tangent volumes"""
    import sdfest_amd.differentiable_renderer as R
    T = 22
    c, depth, target, f10 = scene(name)
    inc = twin.included(depth, target)
    g = shape_information(c, depth, target, T)[0].cpu().numpy()
    up = np.where(inc, depth - target, np.float32(0)).astype(np.float32)
    cam = (c["W"], c["H"], c["cx"], c["cy"], c["fx"], c["fy"])
    g_sdf = hip_backward(R, up, depth, c["sdf"], c["p"], c["q"], [c["inv_scale"]], *cam)[0]
    col = st.tangent_fields().reshape(22, -1) @ g_sdf.reshape(-1).astype(np.float64)
    _, yard = twin.gram(st.joint_features(f10, latent_image(name), T), inc)
    share = np.max(np.abs(g[8:8 + T, 8 + T] - col) / yard[8:8 + T, 8 + T])
    print(f"{name}: latent J^T r against the backward {share:.3e} of sum |s r|")
    assert inc.any() and share <= REL


@pytest.mark.parametrize("T", [1, 8, 22])
def test_sdf_std_matches_float64(T):
    from sdfest_amd import sdf_std
    rng = np.random.default_rng(T)
    K, D = 2, 64 if T == 8 else 9
    Tp = (T + 3) & ~3
    jac = np.zeros((K, D ** 3, Tp), np.float32)
    jac[:, :, :T] = rng.normal(size=(K, D ** 3, T))
    jac[:, :, T:] = np.nan                                  # the padding is not read
    A = rng.normal(size=(K, T, T))
    cov = A @ A.transpose(0, 2, 1) * 1e-3
    cov[1] *= 0.0
    cov[1, 0, 0] = -1.0 if T > 1 else 0.0                   # a negative variance clamps to 0
    got = sdf_std(dev(jac), torch.tensor(cov, device="cuda"))
    assert got.shape == (K, D, D, D) and got.dtype == torch.float32
    j = jac[:, :, :T].astype(np.float64)
    ref = np.sqrt(np.maximum(np.einsum("kva,kab,kvb->kv", j, cov, j), 0.0)).reshape(K, D, D, D)
    err = np.max(np.abs(got.cpu().numpy() - ref)) / ref.max()
    print(f"T={T}: sdf_std {err:.2e} of the largest entry")
    assert err <= 1e-6 and not got[1].any().item()
    assert torch.equal(got, sdf_std(dev(jac), torch.tensor(cov, device="cuda")))
