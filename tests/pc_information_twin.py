"""numpy float64 twin of ``sdfr_pc_information`` and ``sdfr_information_combine`` (test-side only).  Nothing here
imports the product.

Per point the feature vector f = (e0 .. e7, s0 .. s_{T-1}, r, 1) of include/sdfr.h group 19: r the posed SDF at the
point (trilinear, lerp order x, y, z, times scale; 0 outside the volume), e its derivative by (p, raw q, inv_scale),
s_t = scale * trilerp(field t) at the point's cell.  The rotation's derivative is taken from the derivative of the
rotation MATRIX by each quaternion entry, not from the vector identity the kernels use, so that the two statements
check each other."""
import numpy as np


def rotation(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rotation_derivatives(q):
    """(4,3,3): d R / d (x, y, z, w) of the matrix above at q (entries taken as independent)"""
    x, y, z, w = q
    return 2.0 * np.array([[[0, y, z], [y, -2 * x, -w], [z, w, -2 * x]],
                           [[-2 * y, x, w], [x, 0, z], [-w, z, -2 * y]],
                           [[-2 * z, -w, x], [w, -2 * z, y], [x, y, 0]],
                           [[0, -z, y], [z, 0, -x], [-y, x, 0]]])


def grid_coordinates(points, p, q, scale, R):
    """(N,3) float64 grid coordinates of the points in the posed volume, and the pieces they were made of"""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    q = np.asarray(q, np.float64)
    qn = q / np.linalg.norm(q)
    vrel = P - np.asarray(p, np.float64)
    o = vrel @ rotation(qn)                 # rows: R^T vrel
    g = (o / scale + 1.0) * (0.5 * (R - 1))
    return g, o, vrel, qn


def safe_points(points, p, q, scale, R, tol=1e-3):
    """the points whose grid coordinates all stay `tol` away from an integer: next to one the cell, and with it the
    derivative, may differ between fp32 and fp64 (the volume's faces are such coordinates, so inside / outside is
    settled too)"""
    g = grid_coordinates(points, p, q, float(scale), R)[0]
    keep = (np.abs(g - np.round(g)) > tol).all(axis=1)
    return np.asarray(points)[keep]


def _trilinear(vol, cell, off):
    """value and d value / d offset of the (N,) cells of `vol`, lerp x, then y, then z"""
    cx, cy, cz = cell.T
    v = lambda i, j, k: vol[cx + i, cy + j, cz + k]
    ox, oy, oz = off.T
    ax, ay, az = 1 - ox, 1 - oy, 1 - oz
    c00, c01 = v(0, 0, 0) * ax + v(1, 0, 0) * ox, v(0, 0, 1) * ax + v(1, 0, 1) * ox
    c10, c11 = v(0, 1, 0) * ax + v(1, 1, 0) * ox, v(0, 1, 1) * ax + v(1, 1, 1) * ox
    c0, c1 = c00 * ay + c10 * oy, c01 * ay + c11 * oy
    val = c0 * az + c1 * oz
    gx = (((v(1, 0, 0) - v(0, 0, 0)) * ay + (v(1, 1, 0) - v(0, 1, 0)) * oy) * az
          + ((v(1, 0, 1) - v(0, 0, 1)) * ay + (v(1, 1, 1) - v(0, 1, 1)) * oy) * oz)
    gy = (c10 - c00) * az + (c11 - c01) * oz
    gz = c1 - c0
    return val, np.stack([gx, gy, gz], axis=1)


def features(points, p, q, scale, sdf, fields=None, T=0):
    """((N, 10 + T) float64 features, (N,) bool inside)"""
    sdf = np.asarray(sdf, np.float64)
    R = sdf.shape[0]
    scale = float(scale)
    q = np.asarray(q, np.float64)
    g, o, vrel, qn = grid_coordinates(points, p, q, scale, R)
    N = len(g)
    f = np.zeros((N, 10 + T))
    f[:, 9 + T] = 1.0
    cell = np.floor(g)
    inside = ((cell >= 0) & (cell <= R - 2)).all(axis=1) & np.isfinite(g).all(axis=1)
    if not inside.any():
        return f, inside
    c = cell[inside].astype(np.int64)
    off = g[inside] - c
    tri, G = _trilinear(sdf, c, off)
    dvo = G * (0.5 * (R - 1))               # d r / d o:  r = scale tri((o / scale + 1) h - cell)
    oi, vi = o[inside], vrel[inside]
    Rm = rotation(qn)
    e = np.zeros((len(c), 8))
    e[:, 0:3] = -dvo @ Rm.T                 # o = R^T (P - p)
    a = np.stack([np.einsum("ni,ni->n", dvo, vi @ dR) for dR in rotation_derivatives(qn)], axis=1)   # dvo . (dR^T vrel)
    e[:, 3:7] = (a - np.outer(a @ qn, qn)) / np.linalg.norm(q)
    d_scale = tri - np.einsum("ni,ni->n", dvo, oi) / scale
    e[:, 7] = -scale * scale * d_scale      # inv_scale = 1 / scale
    rows = np.zeros((len(c), 10 + T))
    rows[:, :8] = e
    for t in range(T):
        rows[:, 8 + t] = scale * _trilinear(np.asarray(fields[t], np.float64), c, off)[0]
    rows[:, 8 + T] = tri * scale
    rows[:, 9 + T] = 1.0
    f[inside] = rows
    return f, inside


def gram(f):
    """(G = sum_points f f^T, yard = sum_points |f_i f_j|)"""
    a = np.abs(f)
    return f.T @ f, a.T @ a


def combine(gram_depth, gram_pc, K, V, T, pc_weight):
    """include/sdfr.h, sdfr_information_combine, statement by statement: (K V, F, F) float64"""
    F = 10 + T
    gd = np.asarray(gram_depth, np.float64).reshape(K, V, F, F)
    gp = np.asarray(gram_pc, np.float64).reshape(K, V, F, F)
    out = gd.copy()
    w = np.float64(pc_weight)
    for k in range(K):
        cd, cp = np.float64(0.0), np.float64(0.0)
        for v in range(V):
            cd = cd + gd[k, v, F - 1, F - 1]
            cp = cp + gp[k, v, F - 1, F - 1]
        alpha = (w * cd) / cp if (cd > 0 and cp > 0) else np.float64(0.0)
        with np.errstate(invalid="ignore", over="ignore"):
            out[k, :, :F - 1, :F - 1] = gd[k, :, :F - 1, :F - 1] + alpha * gp[k, :, :F - 1, :F - 1]
    return out.reshape(K * V, F, F)
