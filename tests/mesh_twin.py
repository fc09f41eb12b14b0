"""CPU twin of sdfest_amd/csrc/mesh.hip (test-side only; the product never imports it): vectorised numpy marching
cubes with the kernel's ordering contract (include/sdfr.h, group 5), on the case tables ``sdfr_mesh_tables`` returns.
Positions and normals in float64; the crossing decisions compare float32 values with a float32 level, as the
kernel does, so vertex and face lists match it exactly."""
import ctypes

import numpy as np

# edge e = 4 a + m along axis a from corner c0 (corner c = dx + 2 dy + 4 dz)
EDGE_CORNER0 = np.array([0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3])
EDGE_AXIS = np.arange(12) // 4
CORNER_OFF = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)])


def tables():
    """(edge_mask (256,) int, tri_table (256, 16) int) from the library (no GPU needed)"""
    from sdfest_amd import _lib
    em = (ctypes.c_ushort * 256)()
    tt = (ctypes.c_byte * (256 * 16))()
    _lib.check(_lib.lib().sdfr_mesh_tables(ctypes.cast(em, ctypes.c_void_p), ctypes.cast(tt, ctypes.c_void_p)),
               "sdfr_mesh_tables")
    return np.array(em[:], dtype=np.int64), np.array(tt[:], dtype=np.int64).reshape(256, 16)


def padded(sdf, complete):
    sdf = np.asarray(sdf, dtype=np.float32)
    return np.pad(sdf, 1, constant_values=np.float32(1.0)) if complete else sdf


def marching_cubes(sdf, level, complete=False, normals=False, tabs=None):
    """(vertices (V,3) float64, faces (F,3) int64, normals (V,3) float64 or None) of one (R,R,R) grid"""
    edge_mask, tri = tabs if tabs is not None else tables()
    R = sdf.shape[0]
    v = padded(sdf, complete)
    M = v.shape[0]
    lvl = np.float32(level)
    inside = v < lvl
    # crossed owned edges: crossed[i, j, k, a]
    crossed = np.zeros((M, M, M, 3), dtype=bool)
    crossed[:-1, :, :, 0] = inside[:-1] != inside[1:]
    crossed[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    crossed[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = crossed.reshape(-1, 3)
    counts = flat.sum(1)
    vbase = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rank = np.cumsum(flat, axis=1) - flat           # rank of axis a among the point's crossed axes

    g, a = np.nonzero(flat)                          # ascending g, then axis
    idx = np.stack(np.unravel_index(g, (M, M, M)), 1)
    other = idx.copy()
    other[np.arange(len(a)), a] += 1
    va = v[tuple(idx.T)].astype(np.float64)
    vb = v[tuple(other.T)].astype(np.float64)
    t = (np.float64(lvl) - va) / (vb - va)
    pos = idx.astype(np.float64)
    pos[np.arange(len(a)), a] += t
    s = 2.0 / (R - 1)
    verts = (pos - (M - 1) / 2.0) * s

    nrm = None
    if normals:
        grads = np.stack(np.gradient(v.astype(np.float64)), -1)
        ga = grads[tuple(idx.T)]
        gb = grads[tuple(other.T)]
        gn = ga + t[:, None] * (gb - ga)
        ln = np.linalg.norm(gn, axis=1, keepdims=True)
        nrm = np.where(ln > 0, gn / np.where(ln > 0, ln, 1.0), 0.0)

    # cells: case index from the 8 corners
    Mc = M - 1
    case = np.zeros((Mc, Mc, Mc), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = CORNER_OFF[c]
        case |= inside[dx:dx + Mc, dy:dy + Mc, dz:dz + Mc].astype(np.int64) << c
    cells = np.nonzero(case.reshape(-1))[0]
    cases = case.reshape(-1)[cells]
    ntri = (tri[cases] >= 0).sum(1) // 3
    keep = ntri > 0
    cells, cases, ntri = cells[keep], cases[keep], ntri[keep]
    ci = np.stack(np.unravel_index(cells, (Mc, Mc, Mc)), 1)
    cell_g = (ci[:, 0] * M + ci[:, 1]) * M + ci[:, 2]
    e = tri[cases]                                   # (cells, 16), -1 padded
    valid = e >= 0
    ee = np.where(valid, e, 0)
    off = CORNER_OFF[EDGE_CORNER0[ee]]               # (cells, 16, 3)
    owner = cell_g[:, None] + (off[..., 0] * M + off[..., 1]) * M + off[..., 2]
    ax = EDGE_AXIS[ee]
    vid = vbase[owner] + rank[owner, ax]
    faces = vid[valid].reshape(-1, 3)                # row-major: cell ascending, then table order
    return verts, faces.astype(np.int64), nrm


def mesh_area_volume(verts, faces):
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    cr = np.cross(b - a, c - a)
    return 0.5 * np.linalg.norm(cr, axis=1).sum(), np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0


def directed_edges(faces):
    return np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
