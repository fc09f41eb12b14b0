#!/usr/bin/env python3
"""Writes tests/golden/box_iou.npz: 300 seeded pairs of oriented boxes in general position with the volume of their
intersection from scipy (needs scipy; the tests do not).

Per pair: random rotations, side lengths uniform in [0.05, 0.5], the second centre offset from the first by N(0, 0.15^2)
per axis.  The volume: the Chebyshev centre of the 12 half-spaces by ``linprog``; below a radius of 1e-9 the volume is 0,
else ``HalfspaceIntersection`` about that centre -> ``ConvexHull.volume``.  Only general-position pairs go to Qhull:
coplanar, touching and contained boxes are checked by closed forms in the tests.

    boxes_a, boxes_b  (300, 10) float64: centre, quaternion (x, y, z, w), side lengths
    volume            (300,) float64
"""
import os

import numpy as np
from scipy.optimize import linprog
from scipy.spatial import ConvexHull, HalfspaceIntersection
from scipy.spatial.transform import Rotation

PAIRS = 300
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "box_iou.npz")


def halfspaces(box):
    """(6, 4) rows [n, -d]: n.x - d <= 0"""
    c, R, e = box[:3], Rotation.from_quat(box[3:7]).as_matrix(), box[7:]
    rows = []
    for k in range(3):
        for s in (1.0, -1.0):
            n = s * R[:, k]
            rows.append(np.concatenate([n, [-(n @ c + e[k] / 2)]]))
    return np.array(rows)


def scipy_volume(a, b):
    H = np.concatenate([halfspaces(a), halfspaces(b)])
    res = linprog([0, 0, 0, -1], A_ub=np.c_[H[:, :3], np.ones(12)], b_ub=-H[:, 3],
                  bounds=[(None, None)] * 3 + [(0, None)])
    if res.status != 0 or res.x[3] < 1e-9:
        return 0.0
    return float(ConvexHull(HalfspaceIntersection(H, res.x[:3]).intersections).volume)


def main():
    rng = np.random.default_rng(20240607)
    A, B, V = [], [], []
    for i in range(PAIRS):
        ea, eb = rng.uniform(0.05, 0.5, 3), rng.uniform(0.05, 0.5, 3)
        ca = rng.normal(size=3)
        cb = ca + rng.normal(size=3) * 0.15
        qa = Rotation.random(random_state=2 * i).as_quat()
        qb = Rotation.random(random_state=2 * i + 1).as_quat()
        a, b = np.concatenate([ca, qa, ea]), np.concatenate([cb, qb, eb])
        A.append(a), B.append(b), V.append(scipy_volume(a, b))
    V = np.array(V)
    overlapping = int((V > 0).sum())
    assert overlapping >= PAIRS // 2, f"only {overlapping} of {PAIRS} pairs overlap"
    np.savez(OUT, boxes_a=np.array(A), boxes_b=np.array(B), volume=V)
    print(f"{OUT}: {PAIRS} pairs, {overlapping} overlapping, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
