"""CPU: the (7 + T) x (7 + T) algebra of sdfest_amd.uncertainty (joint tangent information, joint covariance) against
its numpy twin (tests/shape_information_twin.py) and against ``pose_covariance`` where the two must agree, the argument
checks of the new C entry points, which run before any HIP call, and the committed fp32 floors of the decoder JVP."""
import ctypes

import numpy as np
import pytest
import torch

import decoder_cases as dc
import information_twin as twin
import shape_information_twin as st
import oracle
from helpers import load_render_case

SCENES = ("g3_pose1_64x48", "g1_sphere_32x24")
T = 5


def joint_gram(name):
    """a joint Gram matrix (10+T, 10+T) of a golden scene: the oracle's pose features and residual of every included
    pixel (test_information_cpu.oracle_gram's set-up), latent features that are seeded smooth functions of the pixel plus
    a share of the pixel's scale derivative (a latent direction that trades against the scale) -- the algebra under test
    does not care where s comes from, only that the matrix is a Gram matrix"""
    c = load_render_case(name)
    cam = (c["cx"], c["cy"], c["fx"], c["fy"])
    render = lambda p, q, s: oracle.render_forward(c["sdf"], p, q, [s], c["W"], c["H"], *cam, c["thr"],
                                                   dtype=np.float32)[0]
    depth = render(c["p"], c["q"], c["inv_scale"])
    target = render(*twin.perturbed_pose(c["p"], c["q"], c["inv_scale"]))
    f = twin.features(depth, target, c["sdf"], c["p"], c["q"], c["inv_scale"], *cam)
    rng = np.random.default_rng(11)
    v, u = np.meshgrid(np.arange(c["H"]) / c["H"], np.arange(c["W"]) / c["W"], indexing="ij")
    s = np.stack([0.05 * np.sin(rng.uniform(10, 40) * u + rng.uniform(10, 40) * v + rng.uniform(0, 6)) for _ in range(T)], -1)
    s[..., 0] += 0.3 * f[..., 7]
    g, _ = twin.gram(st.joint_features(f, s, T), twin.included(depth, target))
    return g, c


@pytest.fixture(scope="module")
def grams():
    return {name: joint_gram(name) for name in SCENES}


def close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) <= rel * max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize("name", SCENES)
def test_joint_tangent_information_matches_the_twin(grams, name):
    from sdfest_amd.uncertainty import joint_tangent_information, tangent_information
    g, c = grams[name]
    q, isc = np.asarray(c["q"], np.float64), c["inv_scale"]
    cam_q = np.array([0.3, -0.2, 0.5, 0.7])
    cam_q /= np.linalg.norm(cam_q)
    for cq in (None, cam_q):
        args = (torch.tensor(q)[None], torch.tensor([isc], dtype=torch.float64), None if cq is None else torch.tensor(cq)[None])
        H = joint_tangent_information(torch.tensor(g)[None], *args)
        assert H.shape == (1, 7 + T, 7 + T) and H.dtype == torch.float64
        assert close(H[0].numpy(), st.joint_tangent_information(g, q, isc, cq))
        # the pose block is tangent_information's, the latent block passes unchanged
        g10 = np.zeros((10, 10))
        g10[:8, :8] = g[:8, :8]
        assert close(H[0, :7, :7].numpy(), tangent_information(torch.tensor(g10)[None], *args)[0].numpy())
        assert close(H[0, 7:, 7:].numpy(), g[8:8 + T, 8:8 + T])
    # two views of one object add
    both = joint_tangent_information(torch.tensor(np.stack([g, g])), torch.tensor(np.stack([q, q])),
                                     torch.tensor([isc, isc], dtype=torch.float64), torch.tensor(np.stack([cam_q, cam_q])))
    assert close(both.sum(0).numpy(), 2.0 * st.joint_tangent_information(g, q, isc, cam_q))


@pytest.mark.parametrize("name", SCENES)
def test_zero_latent_block_without_prior_is_pose_covariance(grams, name):
    from sdfest_amd.uncertainty import pose_covariance, shape_pose_covariance
    g, c = grams[name]
    g10 = np.zeros((10, 10))
    g10[:8, :8] = g[:8, :8]
    H7 = twin.tangent_information(g10, c["q"], c["inv_scale"])
    H = np.zeros((7 + T, 7 + T))
    H[:7, :7] = H7
    rss, cnt = torch.tensor([g[8 + T, 8 + T]]), torch.tensor([g[9 + T, 9 + T]])
    for rcond, sigma in ((1e-6, None), (1e-3, None), (1e-3, 0.002)):
        ref = pose_covariance(torch.tensor(H7)[None], rss, cnt, rcond=rcond, depth_sigma=sigma)
        rec = shape_pose_covariance(torch.tensor(H)[None], rss, cnt, latent_prior=0.0, rcond=rcond, depth_sigma=sigma)
        assert int(rec.rank[0]) == int(ref.rank[0])
        assert close(rec.sigma2.numpy(), ref.sigma2.numpy())
        assert close(rec.pose_covariance[0].numpy(), ref.covariance[0].numpy())
        assert close(rec.conditional.covariance[0].numpy(), ref.covariance[0].numpy(), rel=0.0)
        assert close(rec.position_std.numpy(), ref.position_std.numpy()) and not rec.latent_std.any()


def test_marginal_is_at_least_conditional_and_the_prior_gives_full_rank(grams):
    from sdfest_amd.uncertainty import joint_tangent_information, shape_pose_covariance
    g, c = grams["g3_pose1_64x48"]
    H = joint_tangent_information(torch.tensor(g)[None], torch.tensor(c["q"], dtype=torch.float64)[None],
                                  torch.tensor([c["inv_scale"]], dtype=torch.float64))
    rss, cnt = torch.tensor([g[8 + T, 8 + T]]), torch.tensor([g[9 + T, 9 + T]])
    for prior in (0.0, 1.0, 100.0):
        rec = shape_pose_covariance(H, rss, cnt, latent_prior=prior)
        assert int(rec.conditional.rank[0]) == 7 and int(rec.rank[0]) == 7 + T
        diff = rec.pose_covariance[0].numpy() - rec.conditional.covariance[0].numpy() * float(
            rec.sigma2[0] / rec.conditional.sigma2[0])            # (one sigma2 on both sides: the two ranks differ)
        w = np.linalg.eigvalsh(0.5 * (diff + diff.T))
        assert w.min() >= -1e-12 * w.max(), (prior, w)
        wc = np.linalg.eigvalsh(rec.covariance[0].numpy())
        assert wc.min() >= -1e-12 * wc.max() and np.array_equal(rec.covariance[0].numpy(), rec.covariance[0].numpy().T)
        assert (rec.position_std >= 0).all() and (rec.latent_std > 0).all()
    # a stronger prior narrows the latent, and with it the marginal pose covariance
    weak, strong = (shape_pose_covariance(H, rss, cnt, latent_prior=p) for p in (0.0, 1e6))
    assert (strong.latent_std <= weak.latent_std).all() and (strong.position_std <= weak.position_std * (1 + 1e-9)).all()
    # a latent block of zeros (the observation says nothing about the shape): the prior alone makes the matrix regular
    Hz = H.clone()
    Hz[:, 7:, :] = 0.0
    Hz[:, :, 7:] = 0.0
    rec = shape_pose_covariance(Hz, rss, cnt, latent_prior=1.0)
    assert int(rec.rank[0]) == 7 + T and close(rec.latent_std.numpy(), np.ones((1, T)))
    assert int(shape_pose_covariance(Hz, rss, cnt, latent_prior=0.0).rank[0]) == 7


def test_degenerate_rows_are_reported_not_raised(grams):
    from sdfest_amd.uncertainty import joint_tangent_information, shape_pose_covariance
    g, c = grams["g3_pose1_64x48"]
    H = joint_tangent_information(torch.tensor(g)[None], torch.tensor(c["q"], dtype=torch.float64)[None],
                                  torch.tensor([c["inv_scale"]], dtype=torch.float64))
    rss = torch.tensor([g[8 + T, 8 + T]])
    few = shape_pose_covariance(H, rss, torch.tensor([float(7 + T)]))
    assert torch.isnan(few.sigma2[0]) and torch.isnan(few.covariance[0]).all() and int(few.rank[0]) == 0
    fixed = shape_pose_covariance(H, rss, torch.tensor([float(7 + T)]), depth_sigma=0.001)
    assert torch.isfinite(fixed.covariance).all() and float(fixed.sigma2[0]) == 1e-6
    both = shape_pose_covariance(torch.cat([torch.zeros_like(H), H]), torch.tensor([0.0, float(rss[0])]),
                                 torch.tensor([0.0, g[9 + T, 9 + T]]))
    assert torch.isnan(both.sigma2[0]) and torch.isfinite(both.covariance[1]).all() and int(both.rank[1]) == 7 + T
    nan = shape_pose_covariance(H * float("nan"), rss, torch.tensor([1000.0]))
    assert int(nan.rank[0]) == 0 and torch.isnan(nan.covariance).all()
    sphere, cs = grams["g1_sphere_32x24"]
    Hs = joint_tangent_information(torch.tensor(sphere)[None], torch.tensor(cs["q"], dtype=torch.float64)[None],
                                   torch.tensor([cs["inv_scale"]], dtype=torch.float64))
    rec = shape_pose_covariance(Hs, torch.tensor([sphere[8 + T, 8 + T]]), torch.tensor([sphere[9 + T, 9 + T]]), rcond=1e-3)
    # a sphere's rotation stays unobserved whatever the latent does: the discarded space holds all three rotations
    assert int(rec.conditional.rank[0]) == 4 and 4 <= int(rec.rank[0]) <= 4 + T
    U = rec.unobserved[0].numpy()
    assert int((np.abs(U).sum(1) > 0).sum()) == 7 + T - int(rec.rank[0])
    assert np.sum(np.linalg.svd(U[:, 3:6], compute_uv=False) > 0.9) == 3
    assert torch.isfinite(rec.covariance).all()


def test_one_pixel_image_is_the_one_hot_image():
    """the twin's per-pixel d depth / d SDF: the 1 x 1 image with a moved principal point against the whole one-hot image"""
    for name in ("g3_pose1_64x48", "g4_parallel_slab_33x25"):
        c = load_render_case(name)
        cam = (c["cx"], c["cy"], c["fx"], c["fy"])
        depth = oracle.render_forward(c["sdf"], c["p"], c["q"], [c["inv_scale"]], c["W"], c["H"], *cam, c["thr"],
                                      dtype=np.float32)[0]
        hits = np.argwhere(depth > 0)
        assert len(hits) > 20
        for r, col in hits[:: max(1, len(hits) // 12)]:
            a, b = (st.pixel_sdf_gradient(depth, c["sdf"], c["p"], c["q"], c["inv_scale"], *cam, r, col, whole_image=w)
                    for w in (False, True))
            assert np.count_nonzero(b) in range(1, 9) and np.array_equal(np.flatnonzero(a), np.flatnonzero(b))
            assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), (name, r, col)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from sdfest_amd import _lib
    _lib.build()
    return _lib.lib()


def test_symbols_are_declared_bound_and_exported(L):
    from sdfest_amd import _lib
    vp, i, f, ll, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.c_size_t
    S = _lib.SIGNATURES
    assert S["sdfr_render_information_shape_workspace_bytes"] == (sz, [i, i, i, i])
    assert S["sdfr_render_information_shape"] == (i, [vp, vp, vp, i, ll, vp, i, i, ll, vp, vp, vp, i, i, i, f, f, f, f, f,
                                                      vp, vp, sz, i, vp])
    assert S["sdfr_decoder_jvp_workspace_bytes"] == (sz, [vp, i, i])
    assert S["sdfr_decoder_jvp"] == (i, [vp, vp, vp, vp, vp, i, i, i, vp, vp, sz, vp])
    assert S["sdfr_sdf_std"] == (i, [vp, i, ll, i, i, vp, vp, i, vp])
    for name in ("sdfr_render_information_shape", "sdfr_render_information_shape_workspace_bytes", "sdfr_decoder_jvp",
                 "sdfr_decoder_jvp_workspace_bytes", "sdfr_sdf_std"):
        assert hasattr(L, name), name
    text = open(_lib.HEADER).read()
    contents = text[text.index("CONTENTS"):text.index("#ifndef SDFR_H_")]
    assert contents.index("17. [unstable] DECODER JVP") < contents.index("sdfr_decoder_jvp")
    assert "sdfr_render_information_shape" in contents
    import sdfest_amd
    for name in ("joint_tangent_information", "shape_pose_covariance", "sdf_std", "ShapePoseUncertainty"):
        assert name in sdfest_amd.__all__ and callable(getattr(sdfest_amd, name))
    assert callable(sdfest_amd.SDFDecoder.jvp) and callable(sdfest_amd.SDFVAE.decode_jvp)
    assert callable(sdfest_amd.SDFPipeline.shape_uncertainty)


def test_argument_errors_without_gpu(L):
    from sdfest_amd import _lib
    INVALID, NULL = _lib.ABI["SDFR_E_INVALID"], _lib.ABI["SDFR_E_NULL"]
    err = lambda: L.sdfr_last_error()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)     # a non-NULL pointer that is never dereferenced
    ws = ctypes.c_void_p((q.value + 127) & ~127)
    size = L.sdfr_render_information_shape_workspace_bytes
    # 640 x 480: 10 x 60 tiles of 64 x 8 pixels, a flag word and an 18 x 18 float record each
    assert size(2, 640, 480, 8) == 2 * 600 * 4 + 128 - (2 * 600 * 4) % 128 + 2 * 600 * 18 * 18 * 4
    assert size(1, 33, 25, 1) == 128 + 4 * 121 * 4 and size(1, 33, 25, 22) == 128 + 4 * 1024 * 4
    assert size(0, 8, 8, 8) == 0 and size(1, 0, 8, 8) == 0 and size(65536, 8, 8, 8) == 0
    assert size(1, 8, 8, 0) == 0 and size(1, 8, 8, 23) == 0
    big = 1 << 30
    ok = dict(depth=q, target=q, sdf=q, R=64, stride=0, jac=ws, Tp=8, T=8, jstride=0, pos=q, quat=q, isc=q, B=2, W=32, H=24,
              cx=16.0, cy=12.0, fx=20.0, fy=20.0, thr=0.0, gram=q, ws=ws, bytes=big, device=0, stream=None)
    call = lambda **kw: L.sdfr_render_information_shape(*[kw.get(k, v) for k, v in ok.items()])
    for k in ("depth", "target", "sdf", "jac", "pos", "quat", "isc", "gram", "ws"):
        assert call(**{k: None}) == INVALID and b"sdfr_render_information_shape: NULL" in err(), k
    for kw, msg in ((dict(B=0), b"B=0"), (dict(W=0), b"W=0"), (dict(R=1), b"R=1"), (dict(B=65536), b"B=65536"),
                    (dict(T=0), b"T=0"), (dict(T=23, Tp=24), b"T=23"), (dict(T=-1), b"T=-1"),
                    (dict(Tp=6, T=5), b"Tp=6"), (dict(Tp=4, T=5), b"Tp=4"), (dict(Tp=0, T=1), b"Tp=0"),
                    (dict(jac=ctypes.c_void_p(ws.value + 4)), b"aligned"), (dict(jstride=64 ** 3 * 8 - 4), b"jac_view_stride"),
                    (dict(jstride=64 ** 3 * 8 + 2), b"aligned"), (dict(thr=-0.5), b"inlier_threshold"),
                    (dict(thr=float("nan")), b"inlier_threshold"), (dict(stride=5), b"sdf_view_stride"),
                    (dict(fx=0.0), b"focal"), (dict(bytes=size(2, 32, 24, 8) - 1), b"workspace"),
                    (dict(ws=ctypes.c_void_p(ws.value + 8)), b"aligned")):
        assert call(**kw) == INVALID and msg in err(), (kw, err())
    # sdfr_sdf_std
    std = lambda **kw: L.sdfr_sdf_std(*[kw.get(k, v) for k, v in dict(jac=ws, K=1, voxels=64 ** 3, Tp=8, T=8, cov=q, out=q,
                                                                          device=0, stream=None).items()])
    for kw, msg in ((dict(jac=None), b"NULL"), (dict(cov=None), b"NULL"), (dict(out=None), b"NULL"), (dict(K=0), b"K=0"),
                    (dict(voxels=0), b"voxels=0"), (dict(T=0), b"T=0"), (dict(T=23, Tp=24), b"T=23"), (dict(Tp=6, T=5), b"Tp=6"),
                    (dict(jac=ctypes.c_void_p(ws.value + 4)), b"aligned"), (dict(cov=ctypes.c_void_p(q.value + 4)), b"aligned")):
        assert std(**kw) == INVALID and b"sdfr_sdf_std" in err() and msg in err(), (kw, err())
    # sdfr_decoder_jvp without a handle (the checks that need one run on the GPU: test_decoder_jvp_gpu.py)
    assert L.sdfr_decoder_jvp_workspace_bytes(None, 1, 8) == 0
    assert L.sdfr_decoder_jvp(None, q, q, None, None, 1, 8, 0, ws, ws, big, None) == NULL and b"sdfr_decoder_jvp" in err()


# ---- the committed floors of the decoder JVP ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,T", st.jvp_case_ids())
def test_jvp_floor_is_the_tables(name, T):
    """the table sets the GPU bound: it may not lie above what this CPU measures (one thread) by more than HEADROOM;
    and the float64 statement is a derivative -- a central difference of the float64 decoder agrees with it"""
    stored = st.load_jvp_floors()[name][f"T{T}"]
    v = st.jvp_floor(name, T)
    print(f"{name} T={T}: {v:.2e} (table {stored:.2e})")
    assert stored <= dc.FLOOR and stored <= dc.HEADROOM * v, (name, T, v, stored)
    spec, state, z, tan = st.jvp_inputs(name, T)
    if tan is not None:
        _, ref = st.jvp_reference(name, T)
        eps = 1e-6
        f = lambda zz: dc.walk(spec, state, torch.tensor(zz), torch.float64)[0].numpy()[:, 0]
        z64, t0 = z.astype(np.float64), tan[:, 0].astype(np.float64)
        fd = (f(z64 + eps * t0) - f(z64 - eps * t0)) / (2 * eps)
        assert np.max(np.abs(fd - ref[:, 0])) <= 1e-6 * np.max(np.abs(ref[:, 0])), name
