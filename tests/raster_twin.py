"""CPU twin of the mesh depth rasteriser (csrc/raster.hip, ``sdfr_mesh_depth``): the contract's formulas in vectorised
numpy, float64 by default (test side only, as mesh_twin.py).

Camera at the origin.  Internally x right, y down, z forward (the Open3D / OpenCV frame); a vertex posed in the OpenGL
frame has its y and z negated first.  The ray of pixel (row, col) is d = ((col + 0.5 + ox - cx) / fx,
(row + 0.5 + oy - cy) / fy, 1) with an optional sub-pixel offset (ox, oy); the weight of a vertex is the scalar triple
product d . (p x (q - p)) over the opposite edge, from the edge's vertices in canonical order (lower index p, higher q),
negated for the triangle that walks the edge from q to p; a pixel is covered when the three weights are all >= 0 or all
<= 0 (both faces, inclusive) and their sum is not 0; depth = (w0 z0 + w1 z1 + w2 z2) / (w0 + w1 + w2); the smallest
depth > near wins, the lowest face index among equal depths."""
import numpy as np


def quat_matrix(q):
    x, y, z, w = (float(c) for c in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def pose_vertices(vertices, factor=1.0, quat=(0, 0, 0, 1), position=(0, 0, 0), convention="opengl", dtype=np.float64):
    """R(quat) (factor v) + position in `dtype`, then into the internal frame (y down, z forward)"""
    v = np.asarray(vertices, dtype=dtype)
    R = quat_matrix(quat).astype(dtype)
    p = (v * dtype(factor)) @ R.T + np.asarray(position, dtype=dtype)
    if convention == "opengl":
        p = p * np.array([1, -1, -1], dtype=dtype)
    elif convention not in ("open3d", "opencv"):
        raise ValueError(convention)
    return p.astype(dtype)


def _edge(a, ia, b, ib):
    fwd = (ia < ib)[:, None]
    p, q = np.where(fwd, a, b), np.where(fwd, b, a)
    n = np.cross(p, q - p)
    return np.where(fwd, n, -n)


def render(posed, faces, W, H, fx, fy, cx, cy, near=0.0, offset=(0.0, 0.0), dtype=np.float64, max_pairs=2_000_000):
    """posed (V,3) in the internal frame, faces (F,3) -> depth (H,W) `dtype` (0: no hit), face (H,W) int64 (-1), wmin
    (H,W): the winner's smallest normalised barycentric weight (0 where no hit)"""
    P = np.asarray(posed, dtype=dtype)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    best = np.full(H * W, np.inf, dtype=dtype)
    best_f = np.full(H * W, -1, dtype=np.int64)
    best_w = np.zeros(H * W, dtype=dtype)
    idx = np.arange(len(f))
    ok = ((f >= 0) & (f < len(P))).all(1)
    ok &= (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    f, idx = f[ok], idx[ok]
    with np.errstate(all="ignore"):
        A, B, C = P[f[:, 0]], P[f[:, 1]], P[f[:, 2]]
        ok = np.isfinite(A).all(1) & np.isfinite(B).all(1) & np.isfinite(C).all(1)
        zs = np.stack([A[:, 2], B[:, 2], C[:, 2]], 1)
        ok &= zs.max(1) > 0
        ok &= (np.cross(B - A, C - A) != 0).any(1)
        f, idx, A, B, C, zs = f[ok], idx[ok], A[ok], B[ok], C[ok], zs[ok]
        n0 = _edge(B, f[:, 1], C, f[:, 2])
        n1 = _edge(C, f[:, 2], A, f[:, 0])
        n2 = _edge(A, f[:, 0], B, f[:, 1])
        # conservative pixel boxes (float64 whatever dtype; a pixel of margin covers the sub-pixel offset)
        front = zs.min(1) > 0
        zz = np.where(front[:, None], zs, 1.0).astype(np.float64)
        us = fx * np.stack([A[:, 0], B[:, 0], C[:, 0]], 1).astype(np.float64) / zz + cx - 0.5
        vs = fy * np.stack([A[:, 1], B[:, 1], C[:, 1]], 1).astype(np.float64) / zz + cy - 0.5
        x0 = np.where(front, np.clip(np.floor(us.min(1)) - 1, 0, W), 0).astype(np.int64)
        x1 = np.where(front, np.clip(np.ceil(us.max(1)) + 1, -1, W - 1), W - 1).astype(np.int64)
        y0 = np.where(front, np.clip(np.floor(vs.min(1)) - 1, 0, H), 0).astype(np.int64)
        y1 = np.where(front, np.clip(np.ceil(vs.max(1)) + 1, -1, H - 1), H - 1).astype(np.int64)
    bw, bh = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
    cnt = bw * bh
    sel = np.nonzero(cnt > 0)[0]
    cnt_s = cnt[sel]
    ends = np.cumsum(cnt_s)
    start = 0
    ox, oy = dtype(offset[0]), dtype(offset[1])
    fxd, fyd, cxd, cyd, half = dtype(fx), dtype(fy), dtype(cx), dtype(cy), dtype(0.5)
    while start < len(sel):
        done = ends[start - 1] if start else 0
        stop = int(np.searchsorted(ends, done + max_pairs, side="right"))
        stop = max(stop, start + 1)
        s = sel[start:stop]
        c = cnt[s]
        tri = np.repeat(np.arange(len(s)), c)
        local = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
        t = s[tri]
        col = x0[t] + local % bw[t]
        row = y0[t] + local // bw[t]
        with np.errstate(all="ignore"):
            dx = ((col.astype(dtype) + half + ox) - cxd) / fxd
            dy = ((row.astype(dtype) + half + oy) - cyd) / fyd
            w0 = n0[t, 0] * dx + n0[t, 1] * dy + n0[t, 2]
            w1 = n1[t, 0] * dx + n1[t, 1] * dy + n1[t, 2]
            w2 = n2[t, 0] * dx + n2[t, 1] * dy + n2[t, 2]
            inside = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))
            det = (w0 + w1) + w2
            z = (w0 * zs[t, 0] + w1 * zs[t, 1] + w2 * zs[t, 2]) / det
            hit = inside & (det != 0) & np.isfinite(z) & (z > dtype(near))
            wm = np.minimum(np.minimum(w0 / det, w1 / det), w2 / det)
        pix, z, fi, wm = (row * W + col)[hit], z[hit], idx[t][hit], wm[hit]
        if len(pix):
            order = np.lexsort((fi, z, pix))
            pix, z, fi, wm = pix[order], z[order], fi[order], wm[order]
            first = np.ones(len(pix), dtype=bool)
            first[1:] = pix[1:] != pix[:-1]
            pix, z, fi, wm = pix[first], z[first], fi[first], wm[first]
            better = (z < best[pix]) | ((z == best[pix]) & (fi < best_f[pix]))
            pix, z, fi, wm = pix[better], z[better], fi[better], wm[better]
            best[pix], best_f[pix], best_w[pix] = z, fi, wm
        start = stop
    depth = np.where(best_f >= 0, best, 0).astype(dtype)
    return depth.reshape(H, W), best_f.reshape(H, W), best_w.reshape(H, W)


def camera_params(camera):
    """(W, H, fx, fy, cx, cy) of a ``Camera``, the principal point for pixel centres at 0.5"""
    fx, fy, cx, cy, s = camera.get_pinhole_camera_parameters(0.5)
    assert s == 0
    return int(camera.width), int(camera.height), float(fx), float(fy), float(cx), float(cy)


def render_mesh(mesh, camera, pose, convention="opengl", near=0.0, offset=(0.0, 0.0), dtype=np.float64):
    """mesh = (vertices (V,3), faces (F,3)) in numpy; pose = (factor, quat, position)"""
    v, f = mesh
    posed = pose_vertices(v, pose[0], pose[1], pose[2], convention, dtype)
    return render(posed, f, *camera_params(camera), near=near, offset=offset, dtype=dtype)


def bracket(mesh, camera, pose, eta=1.0 / 32, convention="opengl", near=0.0):
    """The float64 image at the pixel centre and at the four rays displaced by +-eta pixel in x and in y.  Per pixel:
    depth / face / wmin (the centre image), lo / hi (minimum and maximum depth of the five, a miss counting as 0), mixed
    (some of the five hit, some miss), flat (all five hit and hi - lo <= 1e-4 * depth), none (all five miss), all (all
    five hit), face_ok (flat, the five rays hit one and the same triangle, every barycentric weight >= 0.01)"""
    offs = [(0.0, 0.0), (eta, 0.0), (-eta, 0.0), (0.0, eta), (0.0, -eta)]
    imgs = [render_mesh(mesh, camera, pose, convention, near, o) for o in offs]
    d = np.stack([i[0] for i in imgs])
    fc = np.stack([i[1] for i in imgs])
    wm = np.stack([i[2] for i in imgs])
    hit = fc >= 0
    lo, hi = d.min(0), d.max(0)
    all_hit, none = hit.all(0), ~hit.any(0)
    flat = all_hit & (hi - lo <= 1e-4 * d[0])
    face_ok = flat & (fc == fc[0]).all(0) & (wm >= 0.01).all(0)
    return {"depth": d[0], "face": fc[0], "wmin": wm[0], "lo": lo, "hi": hi, "mixed": ~all_hit & ~none, "flat": flat,
            "none": none, "all": all_hit, "face_ok": face_ok}


# ---- small analytic meshes ----------------------------------------------------------------------------------------------
def uv_sphere(n_lat, n_lon, radius=1.0):
    """a closed latitude / longitude sphere: 2 n_lon (n_lat - 1) triangles"""
    th = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    T, Pp = np.meshgrid(th, ph, indexing="ij")
    ring = np.stack([np.sin(T) * np.cos(Pp), np.sin(T) * np.sin(Pp), np.cos(T)], -1).reshape(-1, 3)
    v = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]]) * radius
    i = np.arange(n_lat - 2)[:, None] * n_lon + np.arange(n_lon)[None, :] + 1
    j = np.arange(n_lat - 2)[:, None] * n_lon + (np.arange(n_lon)[None, :] + 1) % n_lon + 1
    quads = np.concatenate([np.stack([i, i + n_lon, j], -1).reshape(-1, 3),
                            np.stack([j, i + n_lon, j + n_lon], -1).reshape(-1, 3)])
    a = np.arange(n_lon)
    top = np.stack([np.zeros(n_lon, int), 1 + a, 1 + (a + 1) % n_lon], -1)
    base = 1 + (n_lat - 2) * n_lon
    bot = np.stack([np.full(n_lon, len(v) - 1), base + (a + 1) % n_lon, base + a], -1)
    return v.astype(np.float32), np.concatenate([top, quads, bot]).astype(np.int32)


def cube(half=1.0):
    """12 triangles, outward winding"""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32) * half
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    return v, f
