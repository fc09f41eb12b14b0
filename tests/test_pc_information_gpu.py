"""GPU: ``sdfr_pc_information`` (through ``sdfest_amd.pc_information``) and ``sdfr_information_combine`` (through
``sdfest_amd.combine_information``) against the float64 twin (tests/pc_information_twin.py).

Against the twin: the back-projected targets of three golden scenes (the target is the HIP forward at the perturbed
pose, tests/test_information_gpu.py's ``scene``; ``oracle.depth_to_pointcloud`` makes the points) at the scene's pose,
T in {0, 1, 8, 22} of ``shape_information_twin.tangent_fields``.  Sizes: seeded points on a perturbed sphere inside an
analytic volume, a tenth of them outside it.  Points with a grid coordinate within 1e-3 of an integer are dropped before
either side sees them (``safe_points``: there fp32 and fp64 may pick different cells); at least 95 % of every set stays.

The bound is tests/test_information_gpu.py's: every entry within REL x sum_points |f_i f_j| of the twin's, REL = 1e-4."""
import functools

import numpy as np
import pytest
import torch

import oracle
import pc_information_twin as tw
import shape_information_twin as st
from test_information_gpu import check_bound, scene
from test_render_gpu import REL, dev

pytestmark = pytest.mark.gpu

SCENES = ("g1_sphere_32x24", "g3_pose1_64x48", "g4_parallel_slab_33x25")
TS = (0, 1, 8, 22)
G = 64      # workgroups per view (sdfest_amd/csrc/pc_information.hip, kPcInfoGroups)
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 256 * G + 1)


def keep_safe(pts, p, q, scale, R):
    kept = tw.safe_points(pts, p, q, scale, R)
    assert len(kept) >= 0.95 * len(pts), (len(pts), len(kept))
    return np.ascontiguousarray(kept, np.float32)


@functools.lru_cache(maxsize=None)
def scene_points(name):
    """(case, points (N,3) float32, scale): the back-projected HIP target of a golden scene"""
    c, _, target, _ = scene(name)
    pts = oracle.depth_to_pointcloud(target, c["fx"], c["fy"], c["cx"] - 0.5, c["cy"] - 0.5, dtype=np.float32)
    scale = float(np.float32(1.0 / c["inv_scale"]))
    assert len(pts) >= 50
    return c, keep_safe(pts, c["p"], c["q"], scale, c["sdf"].shape[0]), scale


@functools.lru_cache(maxsize=None)
def jac_of(T, R=64):
    return dev(st.jac_buffer(st.tangent_fields(R), T))


@functools.lru_cache(maxsize=None)
def analytic_volume(R):
    """(R,R,R) float32: a dented sphere of radius ~0.5 in the volume's [-1, 1]^3"""
    x = np.linspace(-1.0, 1.0, R)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return (np.sqrt(X * X + Y * Y + Z * Z) - 0.5 + 0.05 * np.sin(3 * X + 0.3) * np.cos(2 * Y - Z)).astype(np.float32)


POSE = dict(p=np.array([0.03, -0.02, -0.6]), q=1.2 * np.array([0.2, -0.4, 0.1, 0.88]), scale=0.3)


def sphere_points(M, R, seed, pose=POSE):
    """M seeded points near the surface of ``analytic_volume`` under `pose`, every tenth outside the volume"""
    rng = np.random.default_rng([seed, M, R])
    d = rng.normal(size=(M + 64 + M // 32, 3))      # (room for the ~0.6 % that safe_points drops)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rad = 0.5 * (1.0 + 0.1 * rng.normal(size=len(d)))
    rad[::10] = rng.uniform(1.8, 3.0, size=len(rad[::10]))          # beyond the cube's corner at sqrt(3)
    obj = d * rad[:, None] * pose["scale"]
    world = (obj @ tw.rotation(pose["q"] / np.linalg.norm(pose["q"])).T + pose["p"]).astype(np.float32)
    kept = keep_safe(world, pose["p"], pose["q"], pose["scale"], R)
    assert len(kept) >= M
    return kept[:M]


def information(views, p, q, scale, sdf, T=0, jac=None, single=False, max_view_points=None, workspace=None, R=64):
    """pc_information on numpy inputs: `views` a list of (n,3) point arrays; returns (gram (B,F,F) numpy, inside (B,))"""
    from sdfest_amd import pc_information
    B = len(views)
    pts = dev(np.concatenate(views).astype(np.float32).reshape(-1, 3))
    off = None if single else torch.tensor(np.concatenate([[0], np.cumsum([len(v) for v in views])]), dtype=torch.int32,
                                           device="cuda")
    g, inside = pc_information(pts, off, dev(sdf), dev(np.asarray(p, np.float32).reshape(B, 3)),
                               dev(np.asarray(q, np.float32).reshape(B, 4)), dev(np.asarray(scale, np.float32).reshape(B)),
                               jacobian=(jac_of(T, R) if jac is None else jac) if T else None, tangents=T if T else None,
                               max_view_points=max_view_points, workspace=workspace, return_inside=True)
    assert g.dtype == torch.float64 and g.shape == (B, 10 + T, 10 + T) and g.is_cuda and inside.dtype == torch.int32
    return g, inside


def twin_gram(pts, p, q, scale, sdf, T, R=64, fields=None):
    """the twin at the fp32 values the kernel is handed"""
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    f, inside = tw.features(f32(pts), f32(p), f32(q), float(np.float32(scale)), sdf,
                            st.tangent_fields(R) if fields is None else fields, T)
    return tw.gram(f) + (int(inside.sum()),)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", SCENES)
def test_matches_the_float64_twin(name, T):
    c, pts, scale = scene_points(name)
    g, inside = information([pts], c["p"], c["q"], scale, c["sdf"], T)
    ref, yard, n_in = twin_gram(pts, c["p"], c["q"], scale, c["sdf"], T)
    assert n_in > 0.5 * len(pts)
    check_bound(g[0].cpu().numpy(), ref, yard, f"{name} T={T} ({len(pts)} points, {n_in} inside)")
    assert g[0, 9 + T, 9 + T].item() == len(pts) and inside.tolist() == [n_in]


@pytest.mark.parametrize("M", SIZES)
def test_sizes_around_the_wave_the_block_and_the_group_stride(M):
    T = 1
    sdf = analytic_volume(64)
    pts = sphere_points(M, 64, 1)
    g, inside = information([pts], POSE["p"], POSE["q"], POSE["scale"], sdf, T)
    if M == 0:
        assert not g.any().item() and not torch.signbit(g).any().item() and inside.tolist() == [0]
        return
    ref, yard, n_in = twin_gram(pts, POSE["p"], POSE["q"], POSE["scale"], sdf, T)
    check_bound(g[0].cpu().numpy(), ref, yard, f"M={M}")
    assert g[0, 9 + T, 9 + T].item() == M and inside.tolist() == [n_in]
    assert M < 10 or 0 < n_in < M                                 # both kinds of point are there
    # without offsets (one view of max_view_points points): the same bits
    single, inside1 = information([pts], POSE["p"], POSE["q"], POSE["scale"], sdf, T, single=True)
    assert torch.equal(single, g) and torch.equal(inside1, inside)


@pytest.mark.parametrize("R, T", [(64, 8), (17, 8), (17, 0)])
def test_ragged_batch_with_an_empty_view_and_both_strides(R, T):
    sdf = analytic_volume(R)
    poses = [POSE, dict(p=np.array([-0.05, 0.04, -0.8]), q=np.array([0.5, 0.5, -0.5, 0.5]), scale=0.25),
             dict(p=np.array([0.0, 0.1, -0.5]), q=np.array([-0.3, 0.2, 0.6, 0.7]), scale=0.4)]
    views = [sphere_points(300, R, 2, poses[0]), np.zeros((0, 3), np.float32), sphere_points(65, R, 3, poses[2])]
    P, Q, S = (np.stack([np.asarray(o[k], np.float64) for o in poses]) for k in ("p", "q", "scale"))
    g, inside = information(views, P, Q, S, sdf, T, R=R)
    assert not g[1].any().item() and inside[1].item() == 0
    for b in (0, 2):
        ref, yard, n_in = twin_gram(views[b], P[b], Q[b], S[b], sdf, T, R)
        check_bound(g[b].cpu().numpy(), ref, yard, f"R={R} T={T} view {b}")
        assert g[b, 9 + T, 9 + T].item() == len(views[b]) and inside[b].item() == n_in
    # a volume and a Jacobian per view (sdf_view_stride, jac_view_stride): the same three volumes -> the same bits; then
    # view 2 gets another volume and other fields, and only view 2 changes
    fields = st.tangent_fields(R)
    vols = np.stack([sdf, sdf, sdf])
    jacs = torch.stack([dev(st.jac_buffer(fields, T))] * 3).contiguous() if T else None
    per_view, _ = information(views, P, Q, S, vols, T, jac=jacs, R=R)
    assert torch.equal(per_view, g)
    vols[2] += 0.01
    if T:
        jacs[2] = dev(st.jac_buffer(fields[::-1].copy(), T))
    other, _ = information(views, P, Q, S, vols, T, jac=jacs, R=R)
    assert torch.equal(other[:2], g[:2]) and not torch.equal(other[2], g[2])
    ref, yard, _ = twin_gram(views[2], P[2], Q[2], S[2], vols[2], T, R, fields=fields[::-1])
    check_bound(other[2].cpu().numpy(), ref, yard, f"R={R} T={T} view 2 with its own volume")


@pytest.mark.parametrize("T", [0, 8, 22])
def test_symmetry_reproducibility_and_independence_are_exact(T):
    from sdfest_amd import _lib
    sdf = analytic_volume(64)
    M = 256 * G + 1 if T == 8 else 700
    pts = sphere_points(M, 64, 4)
    args = (POSE["p"], POSE["q"], POSE["scale"], sdf, T)
    g, inside = information([pts], *args)
    assert torch.equal(g, g.transpose(1, 2))
    again, inside2 = information([pts], *args)
    assert torch.equal(g, again) and torch.equal(inside, inside2)
    n = _lib.lib().sdfr_pc_information_workspace_bytes(1, M, T)
    ws = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")            # every word a NaN
    assert torch.equal(g, information([pts], *args, workspace=ws)[0])
    assert torch.equal(g, information([pts], *args, workspace=ws)[0])        # ... and what the call itself left there
    # the view inside a batch of three whose max_view_points is larger
    other = sphere_points(300, 64, 5)
    big = 4 * 256 * G
    P, Q, S = (np.stack([np.asarray(POSE[k], np.float64)] * 3) for k in ("p", "q", "scale"))
    batch, ins = information([other, pts, other[:7]], P, Q, S, sdf, T, max_view_points=big)
    assert torch.equal(batch[1], g[0]) and ins[1].item() == inside[0].item()
    assert torch.equal(batch[0], information([other], *args)[0][0])
    # all points outside the volume: zeros but the count
    far = pts[:300] + np.float32([0, 0, 7.0])
    z, ins = information([far], *args)
    assert z[0, 9 + T, 9 + T].item() == 300 and ins.tolist() == [0]
    z[0, 9 + T, 9 + T] = 0.0
    assert not z.any().item() and not torch.signbit(z).any().item()
    if T:
        # an all-zero Jacobian: exactly zero latent rows and columns, the rest unchanged
        z = information([pts], *args, jac=torch.zeros_like(jac_of(T)))[0][0]
        assert not z[8:8 + T, :].any().item() and not z[:, 8:8 + T].any().item()
        keep = [i for i in range(10 + T) if not 8 <= i < 8 + T]
        assert torch.equal(z[keep][:, keep], g[0][keep][:, keep])


def test_pose_block_of_the_joint_call_meets_the_pose_call():
    T = 8
    c, pts, scale = scene_points("g3_pose1_64x48")
    g = information([pts], c["p"], c["q"], scale, c["sdf"], T)[0][0].cpu().numpy()
    g10 = information([pts], c["p"], c["q"], scale, c["sdf"], 0)[0][0].cpu().numpy()
    _, yard, _ = twin_gram(pts, c["p"], c["q"], scale, c["sdf"], T)
    pick = np.r_[0:8, 8 + T, 9 + T]
    sub, ysub = g[np.ix_(pick, pick)], yard[np.ix_(pick, pick)]
    print(f"T=8 against T=0: {np.max(np.abs(sub - g10) / np.maximum(ysub, 1e-300)):.3e} of sum |f_i f_j|")
    assert np.all(np.abs(sub - g10) <= REL * ysub) and sub[9, 9] == g10[9, 9]


@pytest.mark.parametrize("name", ["g3_pose1_64x48", "g4_parallel_slab_33x25"])
def test_gradient_column_agrees_with_the_samplers_backward(name):
    """the two statements of the per-point derivative: J^T r is sdfr_pc_loss_backward's gradients for the upstream
    gradient r -- g_pos, g_quat, -scale^2 g_scale, and g_sdf contracted with the tangent fields"""
    from sdfest_amd import losses
    T = 22
    c, pts, scale = scene_points(name)
    g = information([pts], c["p"], c["q"], scale, c["sdf"], T)[0][0].cpu().numpy()
    P, pos, quat, sc, vol = (dev(np.asarray(a, np.float32)) for a in (pts, np.reshape(c["p"], (1, 3)), np.reshape(c["q"], (1, 4)),
                                                                      [scale], c["sdf"]))
    r = losses._forward_raw(P, None, len(pts), pos, quat, sc, vol)
    g_sdf, g_pos, g_quat, g_scale = (t.cpu().numpy().astype(np.float64)
                                     for t in losses._backward_raw(r, P, None, len(pts), pos, quat, sc, vol))
    s64 = float(np.float32(scale))
    col = np.concatenate([g_pos[0], g_quat[0], -s64 * s64 * g_scale, st.tangent_fields().reshape(22, -1) @ g_sdf.reshape(-1)])
    _, yard, _ = twin_gram(pts, c["p"], c["q"], scale, c["sdf"], T)
    err, bound = np.abs(g[:8 + T, 8 + T] - col), yard[:8 + T, 8 + T]     # (the slab: a feature that is 0 at every point)
    share = err / np.maximum(bound, 1e-300)
    print(f"{name}: J^T r against the sampler's backward, pose {share[:8].max():.3e}, latent {share[8:].max():.3e} of sum |f r|")
    assert np.all(err <= REL * bound + 1e-300)


def test_combine_information_is_the_twins_bits():
    from sdfest_amd import combine_information
    rng = np.random.default_rng(9)
    K, V, T = 2, 2, 8
    F = 10 + T
    gd, gp = rng.normal(size=(K * V, F, F)), rng.normal(size=(K * V, F, F))
    gd[:, F - 1, F - 1] = [311, 1250, 977, 4]
    gp[:, F - 1, F - 1] = [1000, 1377, 901, 33]
    w = 0.7
    D, P = torch.tensor(gd, device="cuda"), torch.tensor(gp, device="cuda")
    got = combine_information(D, P, V, w)
    assert torch.equal(got.cpu(), torch.tensor(tw.combine(gd, gp, K, V, T, w)))
    assert not torch.equal(got, D) and torch.equal(got[:, F - 1, :], D[:, F - 1, :]) and torch.equal(got[:, :, F - 1], D[:, :, F - 1])
    # an object alone is its row of the pair
    for k in range(K):
        assert torch.equal(combine_information(D[k * V:(k + 1) * V].contiguous(), P[k * V:(k + 1) * V].contiguous(), V, w),
                           got[k * V:(k + 1) * V])
    # no point (cp = 0) or no pixel (cd = 0): the depth term as it is
    for which in (gp, gd):
        a, b = gd.copy(), gp.copy()
        (a if which is gd else b)[:V, F - 1, F - 1] = 0.0
        out = combine_information(torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda"), V, w).cpu()
        assert torch.equal(out, torch.tensor(tw.combine(a, b, K, V, T, w))) and torch.equal(out[:V], torch.tensor(a[:V]))
        assert not torch.equal(out[V:], torch.tensor(a[V:]))
    # in place; T = 0; a NaN propagates
    inplace = D.clone()
    assert combine_information(inplace, P, V, w, out=inplace) is inplace and torch.equal(inplace, got)
    g0, p0 = np.ascontiguousarray(gd[:, :10, :10]), np.ascontiguousarray(gp[:, :10, :10])
    g0[:, 9, 9], p0[:, 9, 9] = gd[:, F - 1, F - 1], gp[:, F - 1, F - 1]
    p0[1, 2, 3] = np.nan
    out0 = combine_information(torch.tensor(g0, device="cuda"), torch.tensor(p0, device="cuda"), 1, 2.0).cpu().numpy()
    assert np.array_equal(out0, tw.combine(g0, p0, 4, 1, 0, 2.0), equal_nan=True) and np.isnan(out0[1, 2, 3])
