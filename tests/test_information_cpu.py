"""CPU: the 7 x 7 algebra of sdfest_amd.uncertainty (tangent map, information, covariance) against its numpy twin
(tests/information_twin.py) on Gram matrices built from the float64 oracle, the facts the algebra rests on (the tangent
map's columns are the first-order steps they claim to be; the quaternion's own direction carries no information; a
sphere's rotation is not observable), and sdfr_render_information's argument checks, which run before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

import information_twin as twin
import oracle
from helpers import load_render_case

SPHERES = ("g1_sphere_32x24", "g1_sphere_64x48", "g4_parallel_slab_33x25")


def oracle_gram(name):
    """Gram matrix of a golden scene from the float64 oracle: estimate = the fp32 oracle's depth at the scene's pose,
    target = its depth at the perturbed pose.  Returns (gram, case)."""
    c = load_render_case(name)
    cam = (c["cx"], c["cy"], c["fx"], c["fy"])
    render = lambda p, q, s: oracle.render_forward(c["sdf"], p, q, [s], c["W"], c["H"], *cam, c["thr"],
                                                   dtype=np.float32)[0]
    depth = render(c["p"], c["q"], c["inv_scale"])
    target = render(*twin.perturbed_pose(c["p"], c["q"], c["inv_scale"]))
    f = twin.features(depth, target, c["sdf"], c["p"], c["q"], c["inv_scale"], *cam)
    g, _ = twin.gram(f, twin.included(depth, target))
    return g, c


@pytest.fixture(scope="module")
def grams():
    return {name: oracle_gram(name) for name in SPHERES + ("g3_pose1_64x48",)}


def test_tangent_map_columns_are_first_order_steps():
    from sdfest_amd.uncertainty import tangent_map
    rng = np.random.default_rng(7)
    for _ in range(8):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        isc = float(rng.uniform(0.5, 4.0))
        T = tangent_map(torch.tensor(q), torch.tensor(isc, dtype=torch.float64))[0].numpy()
        assert np.allclose(T, twin.tangent_map(q, isc), rtol=0, atol=1e-15)
        for k in range(3):
            errs = []
            for eps in (1e-3, 1e-4):
                step = q + eps * T[3:7, 3 + k]
                step /= np.linalg.norm(step)
                w = np.zeros(3)
                w[k] = eps
                exact = twin.qmul(np.concatenate([np.sin(eps / 2) * w / eps, [np.cos(eps / 2)]]), q)
                errs.append(np.max(np.abs(step - exact)))
            assert errs[0] <= 1e-6 and errs[1] <= 1e-8, errs       # O(eps^2) with a constant below 1
            assert errs[1] <= errs[0] * 0.02 + 1e-15, errs          # ... and it does fall a hundredfold
        # log-scale: inv_scale = exp(-s)
        assert np.isclose(T[7, 6], (isc * np.exp(-1e-6) - isc) / 1e-6, rtol=1e-5)
        assert np.array_equal(T[:3, :3], np.eye(3)) and not T[:3, 3:].any() and not T[3:, :3].any()


@pytest.mark.parametrize("name", ["g3_pose1_64x48", "g1_sphere_64x48"])
def test_tangent_information_and_covariance_match_the_twin(grams, name):
    from sdfest_amd.uncertainty import pose_covariance, tangent_information
    g, c = grams[name]
    q, isc = np.asarray(c["q"], np.float64), c["inv_scale"]
    cam_q = np.array([0.3, -0.2, 0.5, 0.7])
    cam_q /= np.linalg.norm(cam_q)
    close = lambda a, b: np.max(np.abs(np.asarray(a) - b)) <= 1e-12 * max(np.max(np.abs(b)), 1e-300)
    for cq in (None, cam_q):
        H7 = tangent_information(torch.tensor(g)[None], torch.tensor(q)[None], torch.tensor([isc], dtype=torch.float64),
                                 None if cq is None else torch.tensor(cq)[None])
        ref = twin.tangent_information(g, q, isc, cq)
        assert H7.shape == (1, 7, 7) and H7.dtype == torch.float64 and close(H7[0].numpy(), ref)
        for rcond, sigma in ((1e-6, None), (1e-3, None), (1e-3, 0.002)):
            rec = pose_covariance(H7, torch.tensor([g[8, 8]]), torch.tensor([g[9, 9]]), rcond=rcond, depth_sigma=sigma)
            t = twin.pose_covariance(ref, g[8, 8], g[9, 9], rcond, sigma)
            assert int(rec.rank[0]) == t["rank"]
            assert close(rec.sigma2[0].numpy(), t["sigma2"]) and close(rec.covariance[0].numpy(), t["covariance"])
            std = np.concatenate([rec.position_std[0].numpy(), np.deg2rad(rec.rotation_std_deg[0].numpy()),
                                  [rec.scale_rel_std[0].item()]])
            assert close(std, t["std"])
            U = rec.unobserved[0].numpy()
            assert int((np.abs(U).sum(1) > 0).sum()) == 7 - t["rank"] and np.allclose(U.T @ U, t["null"], atol=1e-9)
    # the world frame makes views addable: rotating the frame is a congruence, so the spectrum does not move
    w0 = np.linalg.eigvalsh(twin.tangent_information(g, q, isc))
    w1 = np.linalg.eigvalsh(twin.tangent_information(g, q, isc, cam_q))
    assert np.allclose(w0, w1, rtol=1e-9, atol=1e-12 * w0.max())


@pytest.mark.parametrize("name", SPHERES + ("g3_pose1_64x48",))
def test_the_quaternion_norm_is_a_gauge_direction(grams, name):
    g, c = grams[name]
    q = np.asarray(c["q"], np.float64)
    v = np.concatenate([np.zeros(3), q / np.linalg.norm(q), [0.0]])
    assert np.max(np.abs(g[:8, :8] @ v)) <= 1e-12 * np.max(np.abs(g[:8, :8]))


def test_sphere_rank_and_degenerate_rows(grams):
    from sdfest_amd.uncertainty import pose_covariance, tangent_information
    H = []
    for name in SPHERES + ("g3_pose1_64x48",):
        g, c = grams[name]
        H.append(tangent_information(torch.tensor(g)[None], torch.tensor(c["q"], dtype=torch.float64)[None],
                                     torch.tensor([c["inv_scale"]], dtype=torch.float64))[0])
    H = torch.stack(H)
    rss = torch.tensor([grams[n][0][8, 8] for n in SPHERES + ("g3_pose1_64x48",)])
    cnt = torch.tensor([grams[n][0][9, 9] for n in SPHERES + ("g3_pose1_64x48",)])
    # a rotation of a sphere is not observable: position and scale remain
    rec = pose_covariance(H[:3], rss[:3], cnt[:3], rcond=1e-3)
    assert rec.rank.tolist() == [4, 4, 4]
    for k in range(3):
        U = rec.unobserved[k].numpy()
        rot = np.linalg.svd(U[:, 3:6], compute_uv=False)
        assert np.sum(rot > 0.9) == 3                      # the discarded space holds all three rotations
        assert torch.isfinite(rec.covariance[k]).all()
    assert int(pose_covariance(H[3:], rss[3:], cnt[3:], rcond=1e-6).rank[0]) == 7
    # fewer pixels than the rank, and an empty row: reported, not raised
    few = pose_covariance(H[3:], rss[3:], torch.tensor([7.0]))
    assert int(few.rank[0]) == 7 and torch.isnan(few.sigma2[0]) and torch.isnan(few.covariance[0]).all()
    fixed = pose_covariance(H[3:], rss[3:], torch.tensor([7.0]), depth_sigma=0.001)
    assert torch.isfinite(fixed.covariance).all() and float(fixed.sigma2[0]) == 1e-6
    both = pose_covariance(torch.stack([torch.zeros(7, 7, dtype=torch.float64), H[3]]), torch.tensor([0.0, rss[3]]),
                           torch.tensor([0.0, cnt[3]]))
    assert both.rank.tolist() == [0, 7] and torch.isnan(both.sigma2[0]) and torch.isfinite(both.covariance[1]).all()
    assert (np.abs(both.unobserved[0].numpy()).sum(1) > 0).all()      # every direction of the empty row is unobserved
    w = np.linalg.eigvalsh(both.covariance[1].numpy())
    assert w.min() >= -1e-12 * w.max()


@pytest.fixture(scope="module")
def L():
    from sdfest_amd import _lib
    _lib.build()
    return _lib.lib()


def test_symbols_are_declared_bound_and_exported(L):
    from sdfest_amd import _lib
    vp, i, f, ll, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.c_size_t
    assert _lib.SIGNATURES["sdfr_render_information_workspace_bytes"] == (sz, [i, i, i])
    assert _lib.SIGNATURES["sdfr_render_information"] == (i, [vp, vp, vp, i, ll, vp, vp, vp, i, i, i, f, f, f, f, f, vp,
                                                              vp, sz, i, vp])
    for name in ("sdfr_render_information", "sdfr_render_information_workspace_bytes"):
        assert hasattr(L, name), name
    text = open(_lib.HEADER).read()
    contents = text[text.index("CONTENTS"):text.index("#ifndef SDFR_H_")]
    assert contents.index("14. [unstable] POSE INFORMATION") < contents.index("sdfr_render_information")
    import sdfest_amd
    for name in ("render_information", "tangent_information", "pose_covariance"):
        assert name in sdfest_amd.__all__ and callable(getattr(sdfest_amd, name))


def test_argument_errors_without_gpu(L):
    from sdfest_amd import _lib
    INVALID = _lib.ABI["SDFR_E_INVALID"]
    err = lambda: L.sdfr_last_error()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)     # a non-NULL pointer that is never dereferenced
    ws = ctypes.c_void_p((q.value + 127) & ~127)
    size = L.sdfr_render_information_workspace_bytes
    # 640 x 480: 10 x 60 tiles of 64 x 8 pixels, a flag word and a 10 x 10 float record each
    assert size(2, 640, 480) == 2 * 600 * 4 + 128 - (2 * 600 * 4) % 128 + 2 * 600 * 400
    assert size(1, 33, 25) == 128 + 4 * 400
    assert size(0, 8, 8) == 0 and size(1, 0, 8) == 0 and size(1, 8, 0) == 0 and size(65536, 8, 8) == 0
    big = 1 << 30
    ok = dict(depth=q, target=q, sdf=q, R=64, stride=0, pos=q, quat=q, isc=q, B=2, W=32, H=24, cx=16.0, cy=12.0, fx=20.0,
              fy=20.0, thr=0.0, gram=q, ws=ws, bytes=big, device=0, stream=None)
    call = lambda **kw: L.sdfr_render_information(*[kw.get(k, v) for k, v in ok.items()])
    for k in ("depth", "target", "sdf", "pos", "quat", "isc", "gram", "ws"):
        assert call(**{k: None}) == INVALID and b"sdfr_render_information: NULL" in err(), k
    for k, v, msg in (("B", 0, b"B=0"), ("W", 0, b"W=0"), ("H", -1, b"H=-1"), ("R", 0, b"R=0"), ("R", 1, b"R=1"),
                      ("B", 65536, b"B=65536"), ("thr", -0.5, b"inlier_threshold"), ("thr", float("nan"), b"inlier_threshold"),
                      ("thr", float("inf"), b"inlier_threshold"), ("stride", 5, b"sdf_view_stride"),
                      ("fx", 0.0, b"focal"), ("bytes", size(2, 32, 24) - 1, b"workspace"),
                      ("ws", ctypes.c_void_p(ws.value + 8), b"aligned")):
        assert call(**{k: v}) == INVALID and msg in err(), (k, v, err())
