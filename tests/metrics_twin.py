"""numpy twin (no scipy) of sdfest_amd/csrc/metrics.hip: the sampler's Philox stream, triangle choice and barycentrics,
and the brute-force neighbour search with its float32 decision, lowest-index ties and float64 distance."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr (..., 4) uint32, key (2,) uint32 -> (..., 4) uint32 (Random123's Philox-4x32 with 10 rounds)"""
    c = [np.asarray(ctr[..., i], dtype=np.uint32) for i in range(4)]
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = M0 * c[0].astype(np.uint64)
            p1 = M1 * c[2].astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & MASK).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & MASK).astype(np.uint32)
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
            k0 = np.uint32(k0 + W0)
            k1 = np.uint32(k1 + W1)
    return np.stack(c, -1)


def sample_words(n, seed):
    """u (fp64, 53 bits), r1, r2 (fp32, 24 bits) of samples 0 .. n-1"""
    ctr = np.zeros((n, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(n, dtype=np.uint32)
    key = (np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))
    w = philox4x32_10(ctr, key)
    u = ((w[:, 0] >> 5).astype(np.float64) * 67108864.0 + (w[:, 1] >> 6).astype(np.float64)) / 9007199254740992.0
    r1 = (w[:, 2] >> 8).astype(np.float32) * np.float32(1.0 / 16777216.0)
    r2 = (w[:, 3] >> 8).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u, r1, r2


def face_areas(vertices, faces):
    """|(b - a) x (c - a)| in fp64 from the fp32 vertices (the kernel's expression, term by term)"""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    u, w = b - a, c - a
    cx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    cy = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    cz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    return np.sqrt(cx * cx + cy * cy + cz * cz)


def quat_rotate(q, v):
    """v + 2 w (u x v) + 2 u x (u x v) in fp32, operation by operation"""
    q = np.asarray(q, dtype=np.float32)
    u = np.broadcast_to(q[:3], v.shape)
    t = np.cross(u, v).astype(np.float32)
    t2 = np.cross(u, t).astype(np.float32)
    return (v + np.float32(2.0) * (q[3] * t + t2)).astype(np.float32)


def sample_points(vertices, faces, n, seed=0, factor=1.0, quat=(0, 0, 0, 1), position=(0, 0, 0)):
    """(points (n,3) fp32, triangle (n,) int, step_margin (n,) fp64): step_margin is the relative distance of
    u * total to the nearest CDF step (the GPU scans in another order, so choices within ~1e-12 may differ)"""
    v = np.asarray(vertices, dtype=np.float32)
    f = np.asarray(faces, dtype=np.int64)
    cdf = np.cumsum(face_areas(v, f))
    total = cdf[-1]
    u, r1, r2 = sample_words(n, seed)
    target = u * total
    target = np.where(target < total, target, np.nextafter(total, 0.0))
    t = np.searchsorted(cdf, target, side="right")
    lo = np.abs(target - np.where(t > 0, cdf[np.maximum(t - 1, 0)], 0.0))
    hi = np.abs(cdf[t] - target)
    margin = np.minimum(lo, hi) / total
    s = np.sqrt(r1).astype(np.float32)
    wa, wb, wc = np.float32(1) - s, s * (np.float32(1) - r2), s * r2
    A, B, C = v[f[t, 0]], v[f[t, 1]], v[f[t, 2]]
    P = (wa[:, None] * A + wb[:, None] * B + wc[:, None] * C).astype(np.float32)
    P = quat_rotate(quat, np.float32(factor) * P) + np.asarray(position, dtype=np.float32)
    return P.astype(np.float32), t, margin


def _key(d, p):
    d = np.abs(d)
    if p == 2:
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    if p == 1:
        return (d[..., 0] + d[..., 1]) + d[..., 2]
    if np.isinf(p):
        return np.maximum(np.maximum(d[..., 0], d[..., 1]), d[..., 2])
    pp = np.float32(p)
    return (d[..., 0] ** pp + d[..., 1] ** pp) + d[..., 2] ** pp


def dist64(a, b, p):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    if p == 2:
        return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    if p == 1:
        return d[..., 0] + d[..., 1] + d[..., 2]
    if np.isinf(p):
        return np.maximum(np.maximum(d[..., 0], d[..., 1]), d[..., 2])
    return (d[..., 0] ** p + d[..., 1] ** p + d[..., 2] ** p) ** (1.0 / p)


def nearest(queries, refs, p=2, farthest=False, chunk=2048):
    """(fp64 distance, int index) per query: the fp32 key decides (p = 2: the squared sum), ties to the lowest index"""
    q = np.asarray(queries, dtype=np.float32)
    r = np.asarray(refs, dtype=np.float32)
    idx = np.empty(len(q), dtype=np.int64)
    for s in range(0, len(q), chunk):
        k = _key(q[s:s + chunk, None, :] - r[None, :, :], p)
        idx[s:s + chunk] = np.argmax(k, 1) if farthest else np.argmin(k, 1)   # the first extremum
    return dist64(q, r[idx], p), idx
