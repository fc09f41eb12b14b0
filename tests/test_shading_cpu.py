"""CPU: the argument checks of the shading entry points (they refuse before anything touches the GPU), the committed
colour table against matplotlib, the numpy twin against closed forms, and the committed floors."""
import ctypes

import numpy as np
import pytest

import shading_twin as T


@pytest.fixture(scope="module")
def L():
    from sdfest_amd import _lib
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def q():
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)   # a non-NULL, 16-byte aligned pointer that is never dereferenced
    q.keep = buf
    return q


def invalid(L, rc, *words):
    from sdfest_amd import _lib
    msg = L.sdfr_last_error()
    assert rc == _lib.ABI["SDFR_E_INVALID"], (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def normals_call(L, q, depth="q", sdf="q", R=8, stride=0, pos="q", quat="q", isc="q", B=1, W=4, H=4, out="q"):
    p = lambda v: q if v == "q" else v
    return L.sdfr_render_normals(p(depth), p(sdf), R, stride, p(pos), p(quat), p(isc), B, W, H, 2.0, 2.0, 4.0, 4.0,
                                 p(out), 0, None)


def shade_call(L, q, depth="q", sdf="q", R=8, stride=0, pos="q", quat="q", isc="q", B=2, W=4, H=4, V=1, target="q",
               rng="q", rng_stride=0, error_max=0.05, light=(0.0, 0.0, 1.0), background=0xffffff, outs=("q", "q", "q")):
    p = lambda v: q if v == "q" else v
    return L.sdfr_shade_frames(p(depth), p(sdf), R, stride, p(pos), p(quat), p(isc), B, W, H, 2.0, 2.0, 4.0, 4.0, V,
                               p(target), p(rng), rng_stride, error_max, *light, 0.25, 0.2, 0.4, 0.7, background,
                               p(outs[0]), p(outs[1]), p(outs[2]), 0, None)


def test_render_normals_refuses_bad_arguments(L, q):
    for name in ("depth", "sdf", "pos", "quat", "isc", "out"):
        invalid(L, normals_call(L, q, **{name: None}), "sdfr_render_normals", "NULL")
    for name in ("B", "W", "H"):
        for v in (0, -1):
            invalid(L, normals_call(L, q, **{name: v}), "must be positive")
    invalid(L, normals_call(L, q, R=1), "R=1")
    invalid(L, normals_call(L, q, stride=100), "sdf_view_stride")


def test_depth_range_refuses_bad_arguments(L, q):
    invalid(L, L.sdfr_depth_range(None, 1, 4, 4, 0, q, 0, None), "sdfr_depth_range", "NULL")
    invalid(L, L.sdfr_depth_range(q, 1, 4, 4, 0, None, 0, None), "NULL")
    for shape in ((0, 4, 4), (1, 0, 4), (1, 4, -3)):
        invalid(L, L.sdfr_depth_range(q, *shape, 1, q, 0, None), "must be positive")


def test_shade_frames_refuses_bad_arguments(L, q):
    invalid(L, shade_call(L, q, depth=None), "sdfr_shade_frames", "NULL")
    invalid(L, shade_call(L, q, outs=(None, None, None)), "NULL")
    invalid(L, shade_call(L, q, rng=None), "range")               # the depth image needs its range
    invalid(L, shade_call(L, q, target=None), "target")           # the error image its target
    for name in ("sdf", "pos", "quat", "isc"):                    # the shaded image the grid and the poses
        invalid(L, shade_call(L, q, **{name: None}), "shaded_rgb")
    for name in ("B", "W", "H"):
        invalid(L, shade_call(L, q, **{name: 0}), "must be positive")
    invalid(L, shade_call(L, q, R=1), "R=1")
    invalid(L, shade_call(L, q, V=0), "views_per_state=0")
    invalid(L, shade_call(L, q, B=5, V=2), "views_per_state=2", "B=5")
    invalid(L, shade_call(L, q, error_max=0.0), "error_max")
    invalid(L, shade_call(L, q, error_max=-1.0), "error_max")
    invalid(L, shade_call(L, q, error_max=float("nan")), "error_max")
    for s in (1, 3, -2):
        invalid(L, shade_call(L, q, rng_stride=s), f"range_stride={s}")
    invalid(L, shade_call(L, q, light=(0.0, 0.0, 0.0)), "light")
    invalid(L, shade_call(L, q, background=0x1000000), "background")


def test_committed_table_is_matplotlib_viridis():
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps["viridis"].resampled(256)
    expect = np.asarray(cmap(np.arange(256), bytes=True))[:, :3]
    table = T.load_table()
    assert table.shape == (256, 3) and table.dtype == np.uint8
    assert np.array_equal(table, expect)
    # ... and the lookup rule is matplotlib's binning: a normalised value goes through the colormap to the same bytes
    x = np.concatenate([np.linspace(-0.2, 1.2, 1001), (np.arange(256) + 0.5) / 256, [0.0, 1.0]])
    assert np.array_equal(table[T.bins(x)], np.asarray(cmap(x, bytes=True))[:, :3])
    assert 1 <= T.table_step(table) <= 8


PLANE_A = np.array([0.3, -0.5, 0.8])
PLANE_Q = np.array([0.18, -0.31, 0.45, 0.82])
PLANE_Q = PLANE_Q / np.linalg.norm(PLANE_Q)


def plane_sdf(R=8, c=0.1):
    """a . x - c on the R^3 grid over [-1, 1]^3: the trilinear interpolant of a linear field is the field"""
    ax = np.linspace(-1.0, 1.0, R)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return PLANE_A[0] * X + PLANE_A[1] * Y + PLANE_A[2] * Z - c


def test_twin_plane_closed_form():
    """every pixel of ANY depth image has the plane's normal R a / |a|, in whichever cell its hit point falls --
    extrapolating cells outside the grid included"""
    rng = np.random.default_rng(3)
    H, W = 25, 33
    depth = rng.uniform(0.5, 3.0, (H, W))
    depth[rng.random((H, W)) < 0.2] = 0.0
    n, info = T.normals(depth, plane_sdf(), [0.05, -0.1, -1.6], PLANE_Q, 1.3, 16.5, 12.5, 30.0, 29.0)
    expect = T.rotation(PLANE_Q) @ (PLANE_A / np.linalg.norm(PLANE_A))
    hit = depth != 0
    assert np.array_equal(info["hit"], hit)
    assert np.max(np.abs(n[hit] - expect)) < 1e-12
    assert not n[~hit].any()
    # a transposed rotation, a flipped sign or permuted axes would not pass
    assert np.max(np.abs(T.rotation(PLANE_Q).T @ (PLANE_A / np.linalg.norm(PLANE_A)) - expect)) > 0.05
    # the hit point of a pixel lies on its ray at the pixel's depth: camera-frame z of R o + p is -depth
    cam_pts = info["point"] @ T.rotation(PLANE_Q).T + np.array([0.05, -0.1, -1.6])
    assert np.max(np.abs(cam_pts[..., 2][hit] + depth[hit])) < 1e-12


def test_twin_degenerate_gradients_are_zero():
    depth = np.full((4, 5), 1.5)
    for sdf in (np.zeros((8, 8, 8)), np.full((8, 8, 8), np.nan), np.full((8, 8, 8), np.inf)):
        n, info = T.normals(depth, sdf, [0, 0, -1.5], [0, 0, 0, 1], 1.0, 2.5, 2.0, 4.0, 4.0)
        assert not n.any() and not info["valid"].any()


def test_twin_colour_and_range_rules():
    table = T.load_table()
    vmin, vmax = 0.5, 2.5
    centres = vmin + (np.arange(256) + 0.5) / 256 * (vmax - vmin)
    assert np.array_equal(T.depth_bytes(centres[None], vmin, vmax, table)[0], table)
    out = T.depth_bytes(np.array([[0.0, 0.1, 9.0, 1.0]]), vmin, vmax, table)[0]
    assert out[0].tolist() == [255, 255, 255] and np.array_equal(out[1], table[0]) and np.array_equal(out[2], table[255])
    assert np.array_equal(T.depth_bytes(np.array([[1.0, 2.0]]), 1.0, 1.0, table)[0], table[[0, 0]])
    err = T.error_bytes(np.array([[1.0, 1.0, 0.0, 1.0]]), np.array([[1.01, 0.0, 1.0, 3.0]]), 0.05, table)[0]
    assert np.array_equal(err[0], table[51]) and err[1].tolist() == [255] * 3 and err[2].tolist() == [255] * 3
    assert np.array_equal(err[3], table[255])
    assert T.value_range(np.array([0.0, np.nan, np.inf, -np.inf, 2.0, -1.0, 0.5])) == (-1.0, 2.0)
    assert T.value_range(np.zeros((3, 3))) == (0.0, 0.0)
    s = T.shade_bytes(np.array([[[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]]))
    assert s[0, 0].tolist() == [51, 102, 178] and s[0, 1].tolist() == [13, 26, 45]    # full light / the ambient floor


def test_committed_floors_are_current():
    """the floors are what tools/make_shading_floors.py computes (within a factor of 2: numpy versions differ in the
    last bits), for exactly the scenes the GPU test walks"""
    import os
    import sys
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    import make_shading_floors as M
    floors = T.load_floors()
    assert sorted(floors) == sorted(T.TWIN_SCENES)
    for name in T.TWIN_SCENES:
        floor, share = M.scene_floor(name)
        assert 0.5 * floors[name] <= floor <= 2.0 * floors[name], (name, floor, floors[name])
        assert share <= 0.05, (name, share)
        assert floors[name] < 1e-4     # float32's own error is far below what the test allows
