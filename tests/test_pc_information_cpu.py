"""CPU: the float64 twin of the point-cloud information (tests/pc_information_twin.py) against the oracle's sampler and
against central differences, and what of ``sdfr_pc_information`` / ``sdfr_information_combine`` can be asked without a
GPU: the declarations, the argument checks (which run before any HIP call), the workspace sizes, the package's exports.

Points: a golden scene's depth image at the perturbed pose (information_twin.perturbed_pose), back-projected by the
oracle, evaluated at the scene's pose -- what the refiner does with its target."""
import ctypes
import inspect

import numpy as np
import pytest

import information_twin as itw
import oracle
import pc_information_twin as tw
import shape_information_twin as st
from helpers import load_render_case

SCENE = "g3_pose1_64x48"
G = 64      # workgroups per view (sdfest_amd/csrc/pc_information.hip, kPcInfoGroups; include/sdfr.h group 19)


def scene_points(name, dtype=np.float64):
    """(case, points (N,3), scale): the back-projected target of a golden scene, next-to-integer grid coordinates dropped"""
    c = load_render_case(name)
    cam = (c["cx"], c["cy"], c["fx"], c["fy"])
    tp, tq, ts = itw.perturbed_pose(c["p"], c["q"], c["inv_scale"])
    target = oracle.render_forward(c["sdf"], tp, tq, [ts], c["W"], c["H"], *cam, c["thr"], dtype=np.float32)[0]
    pts = oracle.depth_to_pointcloud(target, c["fx"], c["fy"], c["cx"] - 0.5, c["cy"] - 0.5, dtype=np.float32)
    scale = float(np.float32(1.0 / c["inv_scale"]))
    kept = tw.safe_points(pts, c["p"], c["q"], scale, c["sdf"].shape[0])
    assert len(pts) > 100 and len(kept) >= 0.95 * len(pts), (len(pts), len(kept))
    return c, kept.astype(dtype), scale


@pytest.fixture(scope="module")
def case():
    c, pts, scale = scene_points(SCENE)
    # a raw quaternion that is NOT of unit length: the normalisation's Jacobian is part of the features
    q = 1.3 * np.asarray(c["q"], np.float64)
    T = 3
    fields = st.tangent_fields()[:T]
    f, inside = tw.features(pts, c["p"], q, scale, c["sdf"], fields, T)
    return dict(c=c, pts=pts, scale=scale, q=q, T=T, fields=fields, f=f, inside=inside)


def test_residual_is_the_oracles_forward(case):
    c = case["c"]
    ref = oracle.pc_loss_forward(case["pts"], c["p"], case["q"], case["scale"], c["sdf"], dtype=np.float64)
    r = case["f"][:, 8 + case["T"]]
    assert case["inside"].sum() > 100 and np.abs(ref).max() > 0
    assert np.max(np.abs(r - ref)) <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(ref != 0, case["inside"] & (r != 0))
    # points pushed out of the volume: residual 0, no gradient, still counted
    far = case["pts"] + np.array([0.0, 0.0, 5.0])
    f, inside = tw.features(far, c["p"], case["q"], case["scale"], c["sdf"], case["fields"], case["T"])
    assert not inside.any() and not f[:, :-1].any() and (f[:, -1] == 1).all()
    assert not oracle.pc_loss_forward(far, c["p"], case["q"], case["scale"], c["sdf"], dtype=np.float64).any()


def test_weighted_feature_sums_are_the_oracles_backward(case):
    c, f, T, scale = case["c"], case["f"], case["T"], case["scale"]
    go = np.random.default_rng(7).normal(size=len(f))
    g_sdf, g_pos, g_quat, g_scale = oracle.pc_loss_backward(go, case["pts"], c["p"], case["q"], scale, c["sdf"],
                                                            dtype=np.float64)
    got = go @ f
    close = lambda a, b: np.max(np.abs(np.asarray(a) - np.asarray(b))) <= 1e-12 * np.max(np.abs(b))
    assert close(got[0:3], g_pos) and close(got[3:7], g_quat) and close(got[7], -scale * scale * g_scale)
    assert close(got[8:8 + T], case["fields"].reshape(T, -1) @ g_sdf.reshape(-1))


def test_features_are_the_derivatives_of_the_residual(case):
    """central differences of r in p, the raw q, inv_scale and along a tangent field, on the points that stay in their cell"""
    c, f, T, scale, pts = case["c"], case["f"], case["T"], case["scale"], case["pts"]
    p, q, sdf = np.asarray(c["p"], np.float64), case["q"], np.asarray(c["sdf"], np.float64)
    r_of = lambda p_, q_, s_, vol=sdf: tw.features(pts, p_, q_, s_, vol)[0][:, 8]
    eps = 1e-7
    cols = []
    for k in range(3):
        d = np.zeros(3)
        d[k] = eps
        cols.append((r_of(p + d, q, scale) - r_of(p - d, q, scale)) / (2 * eps))
    for k in range(4):
        d = np.zeros(4)
        d[k] = eps
        cols.append((r_of(p, q + d, scale) - r_of(p, q - d, scale)) / (2 * eps))
    isc, di = 1.0 / scale, 1e-6 / scale
    cols.append((r_of(p, q, 1.0 / (isc + di)) - r_of(p, q, 1.0 / (isc - di))) / (2 * di))
    for t in range(T):
        field = case["fields"][t]
        cols.append((r_of(p, q, scale, sdf + 1e-3 * field) - r_of(p, q, scale, sdf - 1e-3 * field)) / 2e-3)
    fd = np.stack(cols, axis=1)
    worst = np.max(np.abs(fd - f[:, :8 + T]), axis=0) / np.max(np.abs(f[:, :8 + T]), axis=0)
    print("central differences against the features, per column, of the column's largest entry:", worst)
    # truncation is O(eps^2), rounding 2^-53 |r| / eps ~ 1e-11 of derivatives of order 1: 1e-6 leaves both far below
    assert worst.max() <= 1e-6


def test_combine_twin_by_hand():
    rng = np.random.default_rng(3)
    K, V, T = 2, 2, 1
    F = 10 + T
    gd, gp = rng.normal(size=(K * V, F, F)), rng.normal(size=(K * V, F, F))
    gd[:, F - 1, F - 1] = [10, 20, 0, 0]         # object 1 has no depth pixel
    gp[:, F - 1, F - 1] = [100, 50, 7, 9]
    out = tw.combine(gd, gp, K, V, T, 0.5)
    alpha = 0.5 * 30 / 150
    assert np.array_equal(out[:2, :F - 1, :F - 1], gd[:2, :F - 1, :F - 1] + alpha * gp[:2, :F - 1, :F - 1])
    assert np.array_equal(out[2:], gd[2:])
    assert np.array_equal(out[:, F - 1, :], gd[:, F - 1, :]) and np.array_equal(out[:, :, F - 1], gd[:, :, F - 1])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from sdfest_amd import _lib
    _lib.build()
    return _lib.lib()


def test_symbols_are_declared_bound_and_exported(L):
    from sdfest_amd import _lib
    vp, i, d, ll, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong, ctypes.c_size_t
    S = _lib.SIGNATURES
    assert S["sdfr_pc_information_workspace_bytes"] == (sz, [i, i, i])
    assert S["sdfr_pc_information"] == (i, [vp, vp, i, i, vp, vp, vp, vp, i, ll, vp, i, i, ll, vp, vp, vp, sz, i, vp])
    assert S["sdfr_information_combine"] == (i, [vp, vp, i, i, i, d, vp, i, vp])
    for name in ("sdfr_pc_information", "sdfr_pc_information_workspace_bytes", "sdfr_information_combine"):
        assert hasattr(L, name), name
    text = open(_lib.HEADER).read()
    contents = text[text.index("CONTENTS"):text.index("#ifndef SDFR_H_")]
    assert contents.index("19. [unstable] POINT-CLOUD INFORMATION") < contents.index("sdfr_pc_information")
    assert "sdfr_information_combine" in contents
    import sdfest_amd
    from sdfest_amd import uncertainty
    for name in ("pc_information", "combine_information"):
        assert name in sdfest_amd.__all__ and getattr(sdfest_amd, name) is getattr(uncertainty, name)
    assert inspect.signature(sdfest_amd.LMRefiner.__init__).parameters["pc_weight"].default == 0.0
    assert inspect.signature(sdfest_amd.SDFPipeline.refine).parameters["pc_weight"].default is None


def test_workspace_sizes(L):
    size = L.sdfr_pc_information_workspace_bytes
    # B min(ceil(M / 256), G) records of (10 + T)^2 floats
    assert size(1, 1, 0) == 1 * 1 * 100 * 4 and size(1, 256, 0) == 100 * 4 and size(1, 257, 0) == 2 * 100 * 4
    assert size(3, 256 * G, 8) == 3 * G * 18 * 18 * 4 == size(3, 256 * G + 1, 8) == size(3, 640 * 480, 8)
    assert size(2, 256 * (G - 1) + 1, 22) == 2 * G * 32 * 32 * 4 and size(2, 256 * (G - 1), 22) == 2 * (G - 1) * 32 * 32 * 4
    assert size(0, 100, 0) == 0 and size(5, 0, 0) == 0                          # nothing to hold
    assert size(-1, 100, 0) == 0 and size(65536, 100, 0) == 0 and size(1, -1, 0) == 0 and size(1, (1 << 30) + 1, 0) == 0
    assert size(1, 100, -1) == 0 and size(1, 100, 23) == 0
    assert size(65535, 1, 22) == 65535 * 1024 * 4


def test_pc_information_argument_errors_without_gpu(L):
    from sdfest_amd import _lib
    INVALID = _lib.ABI["SDFR_E_INVALID"]
    err = lambda: L.sdfr_last_error()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)     # a non-NULL pointer that is never dereferenced
    ws = ctypes.c_void_p((q.value + 127) & ~127)
    size = L.sdfr_pc_information_workspace_bytes
    ok = dict(points=q, offsets=q, B=2, M=1000, pos=q, quat=q, scale=q, sdf=q, R=64, stride=0, jac=ws, Tp=8, T=8, jstride=0,
              gram=q, inside=None, ws=ws, bytes=1 << 30, device=0, stream=None)
    call = lambda **kw: L.sdfr_pc_information(*[kw.get(k, v) for k, v in ok.items()])
    for k in ("points", "pos", "quat", "scale", "sdf", "jac", "gram", "ws"):
        assert call(**{k: None}) == INVALID and b"sdfr_pc_information: NULL" in err(), k
    for kw, msg in ((dict(B=-1), b"B=-1"), (dict(B=65536), b"B=65536"), (dict(M=-1), b"max_view_points=-1"),
                    (dict(M=(1 << 30) + 1), b"max_view_points"), (dict(R=1), b"R=1"), (dict(R=1025), b"R=1025"),
                    (dict(T=23, Tp=24), b"T=23"), (dict(T=-1), b"T=-1"), (dict(Tp=6, T=5), b"Tp=6"),
                    (dict(Tp=4, T=5), b"Tp=4"), (dict(Tp=0, T=1), b"Tp=0"), (dict(stride=5), b"sdf_view_stride"),
                    (dict(jstride=64 ** 3 * 8 - 4), b"jac_view_stride"), (dict(jstride=64 ** 3 * 8 + 2), b"aligned"),
                    (dict(jac=ctypes.c_void_p(ws.value + 4)), b"aligned"), (dict(offsets=None), b"offsets"),
                    (dict(gram=ctypes.c_void_p(q.value + 4)), b"aligned"),
                    (dict(bytes=size(2, 1000, 8) - 1), b"workspace"), (dict(bytes=0), b"workspace"),
                    (dict(ws=ctypes.c_void_p(ws.value + 8)), b"aligned")):
        assert call(**kw) == INVALID and b"sdfr_pc_information" in err() and msg in err(), (kw, err())
    # T = 0: no Jacobian, Tp is not looked at -- the call gets as far as the workspace check
    assert call(T=0, Tp=7, jac=None, bytes=0) == INVALID and b"workspace" in err()
    # nothing to do
    assert call(B=0, points=None, gram=None, ws=None, bytes=0) == 0


def test_combine_argument_errors_without_gpu(L):
    from sdfest_amd import _lib
    INVALID = _lib.ABI["SDFR_E_INVALID"]
    err = lambda: L.sdfr_last_error()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(gd=q, gp=q, K=2, V=2, T=8, w=1.0, out=q, device=0, stream=None)
    call = lambda **kw: L.sdfr_information_combine(*[kw.get(k, v) for k, v in ok.items()])
    for k in ("gd", "gp", "out"):
        assert call(**{k: None}) == INVALID and b"sdfr_information_combine: NULL" in err(), k
    for kw, msg in ((dict(V=65), b"V=65"), (dict(V=0), b"V=0"), (dict(K=0), b"K=0"), (dict(K=65536), b"K=65536"),
                    (dict(T=23), b"T=23"), (dict(T=-1), b"T=-1"), (dict(w=-1.0), b"pc_weight"),
                    (dict(w=float("nan")), b"pc_weight"), (dict(w=float("inf")), b"pc_weight"),
                    (dict(gp=ctypes.c_void_p(q.value + 4)), b"aligned")):
        assert call(**kw) == INVALID and b"sdfr_information_combine" in err() and msg in err(), (kw, err())
