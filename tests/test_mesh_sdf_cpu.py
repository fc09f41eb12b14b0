"""CPU: the float64 twin of sdfr_mesh_sdf (tests/mesh_sdf_twin.py) against analytic fields and the closed-mesh sign
property, and the argument errors of the new entry points and of sdf_utils.mesh_to_sdf (no GPU here)."""
import ctypes

import numpy as np
import pytest

import mesh_sdf_twin as mst
import mesh_twin as mt
import raster_twin as rt


def _grid(R):
    return mst.grid_points(R, np.arange(R ** 3))


def _analytic_scenes():
    sphere = rt.uv_sphere(24, 32, 0.7)
    torus = mst.torus(40, 20, 0.6, 0.25)
    return [("uv_sphere", sphere, lambda p: np.linalg.norm(p.astype(np.float64), axis=1) - 0.7, 0.7),
            ("torus", torus, mst.torus_sdf, 0.25)]   # the last entry: the smallest radius of curvature


@pytest.mark.parametrize("case", _analytic_scenes(), ids=lambda c: c[0])
def test_twin_against_analytic_field(case):
    """The exact field of a mesh inscribed in a smooth surface differs from the surface's own field by at most the
    sagitta of its widest triangle (derived from the mesh, mesh_sdf_twin.sagitta_bound); and what float32 arithmetic
    in the kernel's order loses against float64 is a few roundings of numbers of size <= 4."""
    name, (v, f), field, rho = case
    assert len(f) == {"uv_sphere": 1472, "torus": 1600}[name]
    pts = _grid(24)
    d64, _, w64 = mst.evaluate(pts, v, f)
    inside = w64 > 0.5
    assert np.all(np.abs(w64 - inside) < 1e-9)          # a closed mesh: 0 or 1
    sd = np.where(inside, -d64, d64)
    bound = mst.sagitta_bound(v, f, rho)
    err = np.max(np.abs(sd - field(pts)))
    d32, _, w32 = mst.evaluate(pts, v, f, dtype=np.float32)
    dd, dw = np.max(np.abs(d32.astype(np.float64) - d64)), np.max(np.abs(w32 - w64))
    print(f"{name}: |twin - analytic| {err:.3e} (bound {bound:.3e}); float32 twin: distance {dd:.2e}, winding {dw:.2e}")
    assert err <= bound + 1e-7      # 1e-7: the float32 rounding of the mesh's vertices
    # a dozen roundings (half an ulp each) of intermediate numbers up to 4: 12 * 2^-24 * 2
    assert dd <= 12 * 2.0 ** -24 * 2
    assert np.array_equal(w32 > 0.5, inside)


def test_twin_open_bowl_winding_band():
    """an open mesh: the winding number is a smooth field, and few grid points sit within 1e-3 of the 0.5 level"""
    v, f = mst.bowl()
    assert len(f) == 408
    pts = _grid(24)
    _, _, w64 = mst.evaluate(pts, v, f)
    _, _, w32 = mst.evaluate(pts, v, f, dtype=np.float32)
    band = np.abs(w64 - 0.5) < 1e-3
    print(f"bowl: {band.mean() * 100:.3f} % of 24^3 points within 1e-3 of w = 0.5")
    assert band.mean() < 1e-3
    assert np.array_equal((w32 > 0.5)[~band], (w64 > 0.5)[~band])


def _white_noise(R, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (R, R, R)).astype(np.float32)


def _sphere_grid(R, centre=(0.1, -0.05, 0.08), radius=0.55):
    ax = np.linspace(-1.0, 1.0, R)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - radius).astype(np.float32)


@pytest.mark.parametrize("name, grid", [("sphere", _sphere_grid(12)), ("noise", _white_noise(8, 3)),
                                        ("noise16", _white_noise(16, 4))])
def test_closed_mesh_sign_property(name, grid):
    """A completed marching-cubes mesh is closed and consistently oriented: the winding number is 0 or 1 to 1e-9 at
    every grid point off the surface, and it separates the grid exactly as the level does.  White noise walks through
    all the cases of the table; the share of points ON the surface (|sdf| <= 1e-5, which the GPU separation test
    excludes) stays below that test's 0.5 % cap."""
    R = grid.shape[0]
    v, f, _ = mt.marching_cubes(grid, 0.0, complete=True)
    pts = _grid(R)
    d, _, w = mst.evaluate(pts, v.astype(np.float32), f)
    off = d > 1e-5
    print(f"{name}: {len(f)} faces, {100 * (1 - off.mean()):.3f} % of the grid on the surface")
    assert (~off).mean() <= 0.005
    assert np.all(np.abs(w[off] - np.round(w[off])) <= 1e-9)
    assert set(np.unique(np.round(w[off]))) <= {0.0, 1.0}
    assert np.array_equal((w > 0.5)[off], (grid.reshape(-1) < 0.0)[off])


def test_twin_region_cases_by_hand():
    """one triangle, points over its interior, beside an edge and beyond a vertex; index order and winding of the face
    do not change the distance, the winding number changes sign with the orientation"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    pts = np.array([[0.25, 0.25, 0.5], [0.5, -0.5, 0.0], [-1.0, -1.0, 0.0], [1.0, 1.0, 1.0], [2.0, 0.0, 0.0]], np.float32)
    want = [0.5, 0.5, np.sqrt(2.0), np.sqrt(0.5 + 1.0), 1.0]
    for f in ([[0, 1, 2]], [[1, 2, 0]], [[2, 1, 0]]):
        d, t, w = mst.evaluate(pts, v, np.array(f))
        assert np.allclose(d, want, atol=1e-12) and np.all(t == 0)
        assert np.sign(w[0]) == (1 if f == [[2, 1, 0]] else -1)    # seen from the side the normal points to: w < 0
    # invalid faces contribute nothing; a mesh of nothing else has no distance
    bad = np.array([[0, 0, 1], [0, 1, 7], [0, 1, 3]])
    v4 = np.concatenate([v, [[2, 0, 0]]]).astype(np.float32)      # 0, 1, 3 on a line: zero area
    d, t, w = mst.evaluate(pts, v4, np.concatenate([bad, [[0, 1, 2]]]))
    assert np.allclose(d, want, atol=1e-12) and np.all(t == 3)
    d, t, w = mst.evaluate(pts, v4, bad)
    assert np.all(np.isnan(d)) and np.all(t == -1)


def test_mesh_sdf_argument_errors_without_gpu():
    """argument validation happens before any HIP call"""
    from sdfest_amd import _lib
    _lib.build()
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)   # a non-NULL, 16-byte-aligned-or-not pointer that is never dereferenced
    err = lambda: L.sdfr_last_error()
    assert L.sdfr_mesh_sdf_workspace_bytes(3, 100, 60, 64) == 64 + 100 * 64
    assert L.sdfr_mesh_sdf_workspace_bytes(5, 100, 60, 64) == 128 + 100 * 64
    for bad in ((0, 100, 60, 64), (70000, 100, 60, 64), (1, 0, 0, 64), (1, 100, 101, 64), (1, 100, 0, 64),
                (1, 100, 60, 1), (1, 100, 60, 257)):
        assert L.sdfr_mesh_sdf_workspace_bytes(*bad) == 0, bad
    big = 1 << 30
    assert L.sdfr_mesh_sdf(q, 1, 10, 10, 1, 0, q, None, None, q, big, 0, None) == -1 and b"R=1" in err()
    assert L.sdfr_mesh_sdf(q, 1, 10, 10, 300, 0, q, None, None, q, big, 0, None) == -1 and b"R=300" in err()
    assert L.sdfr_mesh_sdf(q, 0, 10, 10, 64, 0, q, None, None, q, big, 0, None) == -1 and b"K=0" in err()
    assert L.sdfr_mesh_sdf(q, 1, 10, 11, 64, 0, q, None, None, q, big, 0, None) == -1 and b"max_faces" in err()
    assert L.sdfr_mesh_sdf(q, 1, 10, 10, 64, 2, q, None, None, q, big, 0, None) == -1 and b"flags" in err()
    assert L.sdfr_mesh_sdf(q, 1, 10, 10, 64, 1, q, None, q, q, big, 0, None) == -1 and b"winding" in err()
    assert L.sdfr_mesh_sdf(None, 1, 10, 10, 64, 0, q, None, None, q, big, 0, None) == -2
    assert L.sdfr_mesh_sdf(q, 1, 10, 10, 64, 0, None, None, None, q, big, 0, None) == -2
    assert L.sdfr_mesh_sdf(q, 1, 10, 10, 64, 0, q, None, None, None, big, 0, None) == -2 and b"NULL" in err()
    assert L.sdfr_mesh_sdf(q, 1, 10, 10, 64, 0, q, None, None, q, 64, 0, None) == -3 and b"workspace" in err()
    assert (_lib.ABI["SDFR_MESH_SDF_SIGNED"], _lib.ABI["SDFR_MESH_SDF_UNSIGNED"]) == (0, 1)
    vp, i, ll, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
    assert _lib.SIGNATURES["sdfr_mesh_sdf"] == (i, [vp, i, ll, i, i, i, vp, vp, vp, vp, sz, i, vp])
    assert _lib.SIGNATURES["sdfr_mesh_sdf_workspace_bytes"] == (sz, [i, ll, i, i])


def test_mesh_to_sdf_python_errors_without_gpu():
    import torch
    import sdfest_amd
    from sdfest_amd import Mesh, mesh_to_sdf, sdf_utils
    assert sdfest_amd.mesh_to_sdf is sdf_utils.mesh_to_sdf and callable(sdfest_amd.vae_reconstruction)
    tri = Mesh(torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    with pytest.raises(TypeError, match="CUDA"):
        mesh_to_sdf(tri)
    with pytest.raises(TypeError, match="CUDA"):
        tri.to_sdf(32)
    with pytest.raises(ValueError, match="no faces"):
        mesh_to_sdf(Mesh(torch.zeros((3, 3)), torch.zeros((0, 3), dtype=torch.int32)))
    with pytest.raises(ValueError, match="no meshes"):
        mesh_to_sdf([])
    for kw in ({"cells_per_dim": 1}, {"cells_per_dim": 257}, {"padding": -1}, {"cells_per_dim": 8, "padding": 4}):
        with pytest.raises(ValueError):
            mesh_to_sdf(tri, **kw)
    with pytest.raises(ValueError, match="return_winding"):
        mesh_to_sdf(tri, signed=False, return_winding=True)
    # the framing: centre of the bounding box to the origin, the longest extent to 2 (R - 2 p) / R
    v = torch.tensor([[1.0, 2.0, 3.0], [3.0, 2.5, 3.5], [2.0, 6.0, 3.2]])
    s, t = sdf_utils.normalization(v, 64, 4)
    w = v * s + t
    assert torch.allclose(w.amax(0) + w.amin(0), torch.zeros(3), atol=1e-6)
    assert abs(float((w.amax(0) - w.amin(0)).max()) - 2 * 56 / 64) < 1e-6
