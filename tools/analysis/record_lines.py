"""Forward: how many 128-byte lines and 64-byte chunks of the face-record array one march step of a wave touches, for
every candidate record order of unchanged size (16 bytes per voxel).  CPU only: numpy and sdfest_amd.synthetic.

The benchmark's views (blobs_sdf(0), random_poses(256, seed=1), 640 x 480, threshold 0.005) are re-marched with the
kernel's sample sequence: rays that cross the view's may-hit box (plane minima, render.hip setup_box) start on the near
plane of the whole cube and end behind the box; a wave is an 8 x 8-pixel patch; a step of a wave is one iteration in
which at least one of its lanes samples.  Every sample loads the record of its cell's corner (x, y, z) and the record of
(x + 1, y, z).

Per order it prints, per wave-step:
  lines     distinct 128-byte lines over BOTH loads (what the step has to find in L1 or fetch from L2)
  a + b     the same per load, summed (what the two instructions look up)
  chunks    distinct 64-byte chunks per lane quad, summed over the wave's 16 quads and both loads (the unit of the
            gather's data path: DESIGN 3.2)

An order is named by the shape of its line in records, X x Y x Z: [x >> a | y >> b | z >> c | low bits of x, y, z];
its chunks are the squarest halves of the line (ORDERS).
`shipped-r07` is the order until round 7, 1 x 2 x 4; `2x2x2` is the line of the order in device.hpp (record_index puts
x's bits together, [y >> 1 | z >> 1 | x | y & 1 | z & 1]: the same lines and chunks as any other 2 x 2 x 2 order).

    python tools/analysis/record_lines.py [views=16] [first view=0]
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import numpy as np
from sdfest_amd.synthetic import blobs_sdf, random_poses

W, H, F, THR, R = 640, 480, 320.0, 0.005, 64
MAX_STEPS = 4096

# name -> log2 of the extent in (x, y, z) of a 128-byte line (8 records) and of a 64-byte chunk (4 records) inside it
ORDERS = {"shipped-r07 1x2x4": ((0, 1, 2), (0, 1, 1)), "2x2x2": ((1, 1, 1), (0, 1, 1)),
          "4x1x2": ((2, 0, 1), (1, 0, 1)), "4x2x1": ((2, 1, 0), (1, 1, 0)),
          "2x1x4": ((1, 0, 2), (1, 0, 1)), "2x4x1": ((1, 2, 0), (1, 1, 0))}


def block_id(shape, x, y, z):
    """which block of 2^a x 2^b x 2^c records (a line, a chunk) the record of (x, y, z) lies in"""
    a, b, c = shape
    return ((x >> a) * R + (y >> b)) * R + (z >> c)


def rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def sample(sdf, g):
    b = np.clip(np.floor(g), 0, R - 2).astype(np.int64)
    o = g - b
    x, y, z = b[:, 0], b[:, 1], b[:, 2]
    c = lambda dx, dy, dz: sdf[x + dx, y + dy, z + dz]
    c00 = c(0, 0, 0) * (1 - o[:, 0]) + c(1, 0, 0) * o[:, 0]
    c01 = c(0, 0, 1) * (1 - o[:, 0]) + c(1, 0, 1) * o[:, 0]
    c10 = c(0, 1, 0) * (1 - o[:, 0]) + c(1, 1, 0) * o[:, 0]
    c11 = c(0, 1, 1) * (1 - o[:, 0]) + c(1, 1, 1) * o[:, 0]
    c0 = c00 * (1 - o[:, 1]) + c10 * o[:, 1]
    c1 = c01 * (1 - o[:, 1]) + c11 * o[:, 1]
    return c0 * (1 - o[:, 2]) + c1 * o[:, 2], b


def may_hit_box(sdf, p, scale, isc):
    """lo, hi of the view's may-hit box in object units (render.hip, setup_box), None when no slab can hit."""
    h = 0.5 * (R - 1)
    vhit = THR * (np.linalg.norm(p) + 1.7321 * scale) * isc * 1.0001
    cell = scale / h
    lo, hi = np.empty(3), np.empty(3)
    for a in range(3):
        pm = sdf.min(axis=tuple(k for k in range(3) if k != a))
        slabs = np.nonzero(np.minimum(pm[:-1], pm[1:]) < vhit)[0]
        if not len(slabs):
            return None
        lo[a] = max(-scale, (slabs[0] - 0.0625) * cell - scale)
        hi[a] = min(scale, (slabs[-1] + 1 + 0.0625) * cell - scale)
    return lo, hi


def distinct_per_row(ids):
    """ids (n, k) with -1 for idle lanes -> number of distinct ids >= 0 per row"""
    s = np.sort(ids, axis=1)
    return ((s[:, 1:] != s[:, :-1]) & (s[:, 1:] >= 0)).sum(axis=1) + (s[:, 0] >= 0)


def patches(per_pixel):
    """(H * W,) -> (waves, 64): the 8 x 8-pixel patch of every wave, lanes row-major"""
    return per_pixel.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


def main():
    n_views = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    sdf = blobs_sdf(0).astype(np.float64)
    pos, quat, isc_all = random_poses(256, seed=1)
    cols, rows = np.meshgrid(np.arange(W), np.arange(H))
    tot = {k: np.zeros(4) for k in ORDERS}   # union lines, lines of a + lines of b, quad chunks
    wave_steps = 0
    for v in range(first, first + n_views):
        isc = float(isc_all[v]); scale = 1.0 / isc; h = (R - 1) / 2
        Rm = rot(quat[v].astype(np.float64)); p = pos[v].astype(np.float64); e = Rm.T @ p
        box = may_hit_box(sdf, p, scale, isc)
        if box is None:
            continue
        dx = (cols + 0.5 - W / 2) / F; dy = -(rows + 0.5 - H / 2) / F
        d = np.stack([dx, dy, -np.ones_like(dx)], -1); d /= np.linalg.norm(d, axis=-1, keepdims=True)
        dobj = (d @ Rm).reshape(-1, 3)
        with np.errstate(divide="ignore", invalid="ignore"):
            t1 = (e + scale) / dobj; t2 = (e - scale) / dobj          # the whole cube: the march starts on it
            t3 = (e + box[1]) / dobj; t4 = (e + box[0]) / dobj        # the may-hit box: hit or miss, and the far end
        tn = np.maximum(np.minimum(t1, t2).max(-1), 0)
        tn2 = np.minimum(t3, t4).max(-1); tf = np.maximum(t3, t4).min(-1)
        act = (tn2 <= tf) & (tf >= 0) & (tn < tf)
        t = tn.copy()
        og = (-e * isc + 1) * h; dg = dobj * isc * h
        it = 0
        while act.any() and it < MAX_STEPS:
            idx = np.nonzero(act)[0]
            val, bb = sample(sdf, og + t[idx, None] * dg[idx])
            live = patches(act).any(axis=1)
            wave_steps += int(live.sum())
            for name, (line, chunk) in ORDERS.items():
                ids = []
                for shape in (line, chunk):
                    for dx in (0, 1):
                        full = np.full(W * H, -1, np.int64)
                        full[idx] = block_id(shape, bb[:, 0] + dx, bb[:, 1], bb[:, 2])
                        ids.append(patches(full)[live])
                la, lb, ca, cb = ids
                tot[name][0] += distinct_per_row(np.concatenate([la, lb], axis=1)).sum()
                tot[name][1] += distinct_per_row(la).sum() + distinct_per_row(lb).sum()
                for ch in (ca, cb):
                    tot[name][2] += distinct_per_row(ch.reshape(-1, 4)).sum()       # lane quads: 4 consecutive lanes
            dist = val * scale
            hit = dist < THR * t[idx]
            tnew = t[idx] + dist
            stop = hit | ~(tnew < tf[idx])
            t[idx] = np.where(stop, t[idx], tnew)
            act[idx[stop]] = False
            it += 1
    print(f"views {first} .. {first + n_views - 1}: {wave_steps} wave-steps, {wave_steps / n_views:.0f} per view")
    print(f"{'order':20s} {'lines':>7s} {'a + b':>7s} {'chunks':>7s}   (per wave-step; lines vs shipped-r07)")
    base = tot["shipped-r07 1x2x4"][0]
    for name, (u, ab, ch, _) in tot.items():
        print(f"{name:20s} {u / wave_steps:7.2f} {ab / wave_steps:7.2f} {ch / wave_steps:7.2f}   {100 * (u / base - 1):+6.1f} %")


if __name__ == "__main__":
    main()
