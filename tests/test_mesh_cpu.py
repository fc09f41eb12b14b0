"""CPU: the marching-cubes case tables of sdfest_amd/csrc/mesh.hip (read through ``sdfr_mesh_tables``, no GPU) are
crack-free and consistently wound for all 256 cases; the CPU twin (tests/mesh_twin.py) built on them gives closed,
oriented meshes on a sphere, the decoded mug and white noise; the MESH group of the C ABI validates its arguments
before any HIP call."""
import ctypes
import os

import numpy as np
import pytest

from helpers import GOLDEN
import mesh_twin as mt

CORNERS = mt.CORNER_OFF
EDGE_C0 = mt.EDGE_CORNER0
EDGE_C1 = EDGE_C0 | (1 << mt.EDGE_AXIS)
# the six faces as (axis, side): the edges lying in a face have both corners on it
FACES = [(a, s) for a in range(3) for s in (0, 1)]


def on_face(e, face):
    a, s = face
    return CORNERS[EDGE_C0[e], a] == s and CORNERS[EDGE_C1[e], a] == s


def face_pattern(case, face):
    a, s = face
    return tuple((case >> c) & 1 for c in range(8) if CORNERS[c, a] == s)


@pytest.fixture(scope="module")
def tabs():
    return mt.tables()


def triangles(tri, case):
    t = tri[case]
    t = t[t >= 0]
    assert len(t) % 3 == 0
    return t.reshape(-1, 3)


def crossed_edges(case):
    return {e for e in range(12) if ((case >> EDGE_C0[e]) & 1) != ((case >> EDGE_C1[e]) & 1)}


def boundary(tris):
    """the directed triangle edges whose reverse is not in the case's own triangles (multiset difference)"""
    from collections import Counter
    cnt = Counter()
    for a, b, c in tris:
        for u, v in ((a, b), (b, c), (c, a)):
            if cnt[(v, u)]:
                cnt[(v, u)] -= 1
            else:
                cnt[(u, v)] += 1
    return sorted(k for k, n in cnt.items() for _ in range(n))


def test_tables_use_exactly_the_crossed_edges(tabs):
    edge_mask, tri = tabs
    for case in range(256):
        used = set(triangles(tri, case).reshape(-1).tolist())
        assert used == crossed_edges(case), case
        assert edge_mask[case] == sum(1 << e for e in crossed_edges(case)), case
        assert (tri[case][len(triangles(tri, case)) * 3:] == -1).all()
    assert max(len(triangles(tri, c)) for c in range(256)) <= 5


def test_winding_agrees_with_corner_signs(tabs):
    """every triangle has an uncancelled edge on a cube face (a fan from a loop of face segments), and on that face it runs
    with the inside ends of its two cube edges on its right and the outside ends on its left, seen from outside the
    cube: so
    (b-a) x (c-a) points toward increasing SDF.  Checked on the edge midpoints for every triangle of every case."""
    _, tri = tabs
    mid = (CORNERS[EDGE_C0] + CORNERS[EDGE_C1]) / 2.0
    for case in range(1, 255):
        segs = set(boundary(triangles(tri, case)))
        for a, b, c in triangles(tri, case):
            checked = 0
            for u, v in ((a, b), (b, c), (c, a)):
                if (u, v) not in segs:       # a fan diagonal, cancelled inside the cube
                    continue
                for (ax, side) in FACES:
                    if not (on_face(u, (ax, side)) and on_face(v, (ax, side))):
                        continue
                    normal = np.zeros(3)
                    normal[ax] = 1.0 if side else -1.0
                    for corner in (EDGE_C0[u], EDGE_C1[u], EDGE_C0[v], EDGE_C1[v]):   # the corners it separates
                        turn = np.dot(np.cross(mid[v] - mid[u], CORNERS[corner] - mid[u]), normal)
                        inside = (case >> corner) & 1
                        assert (turn < 0) if inside else (turn > 0), (case, (a, b, c), corner)
                    checked += 1
            assert checked >= 1, (case, (a, b, c))


def test_uncancelled_boundary_lies_on_cube_faces(tabs):
    _, tri = tabs
    for case in range(256):
        for u, v in boundary(triangles(tri, case)):
            assert sum(on_face(u, f) and on_face(v, f) for f in FACES) == 1, (case, u, v)


def face_segments(tri, case, face):
    return sorted((u, v) for u, v in boundary(triangles(tri, case)) if on_face(u, face) and on_face(v, face))


def test_face_segments_depend_on_the_face_signs_alone_and_match_the_neighbour(tabs):
    """on each face, the boundary segments are a function of that face's four corner signs; the neighbouring cube,
    which has the same face as its opposite side, sees the same segments reversed.  With the two tests above this
    makes every mesh of the table closed and consistently oriented, for any field."""
    _, tri = tabs
    seen = {}
    for case in range(256):
        for face in FACES:
            key = (face, face_pattern(case, face))
            segs = face_segments(tri, case, face)
            assert seen.setdefault(key, segs) == segs, (case, face)
    assert len(seen) == 6 * 16
    for a in range(3):
        for pattern in {k[1] for k in seen if k[0] == (a, 1)}:
            hi = seen[((a, 1), pattern)]
            lo = seen[((a, 0), pattern)]     # the same four signs on the neighbour's low face
            # an edge on the high face maps to the neighbour's edge with that axis' offset 0: clear the bit of `a`
            moved = []
            for u, v in hi:
                mu = [e for e in range(12) if EDGE_C0[e] == EDGE_C0[u] & ~(1 << a) and mt.EDGE_AXIS[e] == mt.EDGE_AXIS[u]]
                mv = [e for e in range(12) if EDGE_C0[e] == EDGE_C0[v] & ~(1 << a) and mt.EDGE_AXIS[e] == mt.EDGE_AXIS[v]]
                moved.append((mv[0], mu[0]))     # reversed
            assert sorted(moved) == lo, (a, pattern)


def closed_and_oriented(faces):
    de = mt.directed_edges(faces)
    n = int(faces.max()) + 1
    fwd, cf = np.unique(de[:, 0] * n + de[:, 1], return_counts=True)
    rev, cr = np.unique(de[:, 1] * n + de[:, 0], return_counts=True)
    return np.array_equal(fwd, rev) and np.array_equal(cf, cr), len(fwd)


def fields():
    from sdfest_amd.synthetic import sphere_sdf
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    noise = np.random.default_rng(0).uniform(-1, 1, (32, 32, 32)).astype(np.float32)
    return {"sphere": (sphere_sdf(0.5, 64), 0.0), "mug": (d["z0_full"], 0.02), "noise": (noise, 0.0)}


@pytest.mark.parametrize("name", ["sphere", "mug", "noise"])
def test_twin_complete_meshes_are_closed_and_oriented(tabs, name):
    sdf, level = fields()[name]
    v, f, _ = mt.marching_cubes(sdf, level, complete=True, tabs=tabs)
    ok, n_edges = closed_and_oriented(f)
    assert ok
    assert not np.any((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]))
    assert len(v) == len(np.unique(f))        # every vertex is used
    if name == "mug":
        assert 18000 < len(v) < 20000 and np.abs(v).max() < 1.0    # one inside component away from the border
    if name == "noise":      # every case, many times
        inside = mt.padded(sdf, True) < 0
        cases = sum(inside[(c & 1):(c & 1) + 33, (c >> 1 & 1):(c >> 1 & 1) + 33, (c >> 2 & 1):(c >> 2 & 1) + 33]
                    .astype(int) << c for c in range(8))
        assert len(np.unique(cases)) == 256 and len(f) > 100000


def test_twin_sphere_topology_area_volume_normals(tabs):
    from sdfest_amd.synthetic import sphere_sdf
    v, f, n = mt.marching_cubes(sphere_sdf(0.5, 64), 0.0, complete=True, normals=True, tabs=tabs)
    _, n_edges = closed_and_oriented(f)
    assert len(v) - n_edges // 2 + len(f) == 2
    area, vol = mt.mesh_area_volume(v, f)
    r = 0.5
    # measured: -0.13 % and -0.24 %
    assert abs(area / (4 * np.pi * r * r) - 1) < 0.01
    assert abs(vol / (4.0 / 3.0 * np.pi * r ** 3) - 1) < 0.01
    radial = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert np.min(np.einsum("ij,ij->i", radial, n)) >= 0.999     # measured: 0.9999996
    assert np.abs(np.linalg.norm(v, axis=1) - r).max() < 1e-3


def test_twin_positions_are_the_reference_frame(tabs):
    """an unpadded R^3 grid maps to [-1, 1]; with `complete`, padded index i lands at (i - 1) s - 1"""
    R = 8
    sdf = np.full((R, R, R), 1.0, dtype=np.float32)
    sdf[0, 0, 0] = -1.0                      # one inside corner at the grid's origin
    v, f, _ = mt.marching_cubes(sdf, 0.0, tabs=tabs)
    s = 2.0 / (R - 1)
    np.testing.assert_allclose(v, [[-1 + 0.5 * s, -1, -1], [-1, -1 + 0.5 * s, -1], [-1, -1, -1 + 0.5 * s]])
    assert f.tolist() == [[0, 1, 2]]
    vc, fc, _ = mt.marching_cubes(sdf, 0.0, complete=True, tabs=tabs)
    assert len(vc) == 6 and len(fc) == 8     # the corner, closed by the border: an octahedron


@pytest.fixture(scope="module")
def L():
    from sdfest_amd import _lib
    _lib.build()
    return _lib.lib()


def test_mesh_abi_argument_errors_without_gpu(L):
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)    # a non-NULL pointer that is never dereferenced
    err = lambda: L.sdfr_last_error()
    assert L.sdfr_mesh_workspace_bytes(1, 1, 0) == 0
    assert L.sdfr_mesh_workspace_bytes(0, 64, 0) == 0
    # partials {V, F, min, max} per 256 points + one word per point
    assert L.sdfr_mesh_workspace_bytes(2, 64, 0) == 2 * (64 ** 3 // 256) * 16 + 2 * 64 ** 3 * 4
    assert L.sdfr_mesh_workspace_bytes(1, 64, 1) == ((66 ** 3 + 255) // 256) * 16 + 66 ** 3 * 4
    big = 1 << 30
    assert L.sdfr_mesh_count(q, 1, 1, 0, 0.0, q, q, big, 0, None) == -1 and b"R=1" in err()
    assert L.sdfr_mesh_count(q, 1, 257, 0, 0.0, q, q, big, 0, None) == -1 and b"R=257" in err()
    assert L.sdfr_mesh_count(q, 0, 64, 0, 0.0, q, q, big, 0, None) == -1 and b"N=0" in err()
    assert L.sdfr_mesh_count(q, 1, 64, 2, 0.0, q, q, big, 0, None) == -1 and b"complete" in err()
    assert L.sdfr_mesh_count(None, 1, 64, 0, 0.0, q, q, big, 0, None) == -2
    assert L.sdfr_mesh_count(q, 1, 64, 0, 0.0, None, q, big, 0, None) == -2
    assert L.sdfr_mesh_count(q, 1, 64, 0, 0.0, q, None, big, 0, None) == -2
    assert L.sdfr_mesh_count(q, 1, 64, 0, 0.0, q, q, 64, 0, None) == -3 and b"workspace" in err()
    assert L.sdfr_mesh_emit(q, 1, 1, 0, 0.0, q, q, None, q, q, big, 0, None) == -1 and b"R=1" in err()
    assert L.sdfr_mesh_emit(q, -3, 64, 0, 0.0, q, q, None, q, q, big, 0, None) == -1
    assert L.sdfr_mesh_emit(q, 1, 64, 0, 0.0, q, None, None, q, q, big, 0, None) == -2
    assert L.sdfr_mesh_emit(q, 1, 64, 0, 0.0, q, q, None, None, q, big, 0, None) == -2
    assert L.sdfr_mesh_emit(q, 1, 64, 0, 0.0, None, q, None, q, q, big, 0, None) == -2
    assert L.sdfr_mesh_emit(q, 1, 64, 0, 0.0, q, q, None, q, q, 16, 0, None) == -3
    assert L.sdfr_mesh_tables(None, q) == -2


def test_mesh_module_rejects_cpu_tensors():
    import torch
    from sdfest_amd import extract_mesh
    with pytest.raises(TypeError):
        extract_mesh(torch.zeros(8, 8, 8), 0.0)
    with pytest.raises(ValueError):
        extract_mesh(torch.zeros(2, 3, 8, 8, 8), 0.0)


def test_library_tables_are_the_generator_output(tabs):
    """sdfest_amd/csrc/mesh_tables.hpp is what tools/gen_mesh_tables.py derives (the header is generated, not edited)"""
    import importlib.util
    from helpers import ROOT
    spec = importlib.util.spec_from_file_location("gen_mesh_tables", os.path.join(ROOT, "tools", "gen_mesh_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    edge_mask, tri = gen.tables()
    assert np.array_equal(tabs[0], edge_mask) and np.array_equal(tabs[1], np.array(tri))
    assert [c0 for c0, _, _ in gen.EDGES] == list(mt.EDGE_CORNER0)
