#!/usr/bin/env python3
"""Capture tests/golden/metrics.npz by IMPORTING the reference's sdfest/estimation/metrics.py (numpy + scipy; dev
container only; loaded by file path, the package's __init__ pulls in open3d).

Every point set is float32-valued, so the GPU's float32 inputs are exactly scipy's float64 inputs.  Cases: a noisy
sphere pair (N != M), 1 vs many and many vs 1, a lattice with duplicated points and exact ties, and a hand-checkable
triple; for p in {1, 2, inf, 3} and normalize off / on: every point metric at every threshold of the case, scipy's
per-point distances, and extent.  correct_thresh on seeded poses.  The tool refuses to write a golden whose distance
lies within 1e-5 relative of a tested threshold, so threshold metrics compare exactly.

Usage:  python tools/make_metric_goldens.py [--ref /root/reference]
"""
import argparse
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "metrics.npz")
P_NORMS = {"1": 1, "2": 2, "inf": np.inf, "3": 3}
MARGIN = 1e-5


def load_metrics(ref):
    path = os.path.join(ref, "sdfest/estimation/metrics.py")
    spec = importlib.util.spec_from_file_location("ref_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sphere(rng, n, r, noise):
    x = rng.normal(size=(n, 3))
    x = r * x / np.linalg.norm(x, axis=1, keepdims=True) + rng.normal(scale=noise, size=(n, 3))
    return x.astype(np.float32)


def cases():
    rng = np.random.default_rng(11)
    lattice = np.stack(np.meshgrid(*[np.arange(4) * 0.25] * 3, indexing="ij"), -1).reshape(-1, 3)
    return {
        # name: (gt, rec, raw thresholds, normalised thresholds)
        "sphere": (sphere(rng, 700, 0.1, 0.002), sphere(rng, 500, 0.104, 0.004), [0.01, 0.004], [0.05, 0.02]),
        "one_vs_many": (sphere(rng, 1, 0.1, 0.0), sphere(rng, 65, 0.1, 0.01), [0.1, 0.15], [0.1]),
        "many_vs_one": (sphere(rng, 63, 0.1, 0.01), sphere(rng, 1, 0.1, 0.0), [0.1, 0.15], [0.5, 0.9]),
        # every rec point lies exactly between two lattice points; every gt point is there twice
        "ties": (np.concatenate([lattice, lattice]).astype(np.float32),
                 (lattice + np.array([0.125, 0.0, 0.0])).astype(np.float32), [0.2, 0.1], [0.05, 0.2]),
        "hand": (np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32),
                 np.array([[0, 0, 0.5], [1, 0, 0]], np.float32), [0.25, 1.0], [0.1, 0.3]),
    }


def check_margin(d, thresholds, what):
    for t in thresholds:
        near = np.abs(d - t) <= MARGIN * t
        assert not near.any(), f"{what}: distance {d[near][0]} within {MARGIN} relative of threshold {t}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    m = load_metrics(a.ref)
    import scipy.spatial
    from scipy.spatial.transform import Rotation

    out = {"p_names": np.array(list(P_NORMS)), "case_names": np.array(list(cases()))}
    for name, (gt, rec, t_raw, t_norm) in cases().items():
        assert gt.dtype == rec.dtype == np.float32
        out[f"{name}/gt"], out[f"{name}/rec"] = gt, rec
        out[f"{name}/t_raw"], out[f"{name}/t_norm"] = np.array(t_raw), np.array(t_norm)
        ext = m.extent(gt.astype(np.float64))
        out[f"{name}/extent"] = np.float64(ext)
        for pn, p in P_NORMS.items():
            g, r = gt.astype(np.float64), rec.astype(np.float64)
            d_acc, _ = scipy.spatial.KDTree(g).query(r, p=p)
            d_comp, _ = scipy.spatial.KDTree(r).query(g, p=p)
            out[f"{name}/p{pn}/d_acc"], out[f"{name}/p{pn}/d_comp"] = d_acc, d_comp
            for d in (d_acc, d_comp):
                check_margin(d, t_raw, f"{name} p={pn}")
                check_margin(d / ext, t_norm, f"{name} p={pn} normalised")
            for nz, ts in ((0, t_raw), (1, t_norm)):
                key = f"{name}/p{pn}/n{nz}"
                kw = dict(p_norm=p, normalize=bool(nz))
                out[f"{key}/mean_accuracy"] = np.float64(m.mean_accuracy(g, r, **kw))
                out[f"{key}/mean_completeness"] = np.float64(m.mean_completeness(g, r, **kw))
                out[f"{key}/symmetric_chamfer"] = np.float64(m.symmetric_chamfer(g, r, **kw))
                out[f"{key}/accuracy_thresh"] = np.array([m.accuracy_thresh(g, r, t, **kw) for t in ts], np.float64)
                out[f"{key}/completeness_thresh"] = np.array([m.completeness_thresh(g, r, t, **kw) for t in ts],
                                                             np.float64)
                out[f"{key}/reconstruction_fscore"] = np.array([m.reconstruction_fscore(g, r, t, **kw) for t in ts],
                                                               np.float64)

    # correct_thresh: seeded poses, every threshold combination; quaternions scalar-last
    rng = np.random.default_rng(5)
    rows = []
    for i in range(24):
        q_gt = Rotation.random(random_state=100 + i)
        q_pr = Rotation.from_rotvec(rng.normal(scale=0.15, size=3)) * q_gt
        p_gt = rng.normal(scale=0.3, size=3)
        p_pr = p_gt + rng.normal(scale=0.02, size=3)
        pos_thr = [None, 0.02, 0.05][i % 3]
        deg_thr = [None, 5.0, 10.0][(i // 3) % 3]
        axis = [None, 1][(i // 9) % 2]
        res = m.correct_thresh(p_gt, p_pr, q_gt, q_pr, position_threshold=pos_thr, degree_threshold=deg_thr,
                               rotational_symmetry_axis=axis)
        rows.append((q_gt.as_quat(), q_pr.as_quat(), p_gt, p_pr, np.nan if pos_thr is None else pos_thr,
                     np.nan if deg_thr is None else deg_thr, -1 if axis is None else axis, res))
    out["correct/q_gt"] = np.array([r[0] for r in rows])
    out["correct/q_pred"] = np.array([r[1] for r in rows])
    out["correct/p_gt"] = np.array([r[2] for r in rows])
    out["correct/p_pred"] = np.array([r[3] for r in rows])
    out["correct/position_threshold"] = np.array([r[4] for r in rows])
    out["correct/degree_threshold"] = np.array([r[5] for r in rows])
    out["correct/axis"] = np.array([r[6] for r in rows], np.int64)
    out["correct/result"] = np.array([r[7] for r in rows], np.int64)
    gt, rec = cases()["sphere"][:2]
    ident = Rotation.identity()
    out["correct/fscore_thresholds"] = np.array([0.3, 0.9])
    out["correct/fscore_result"] = np.array([m.correct_thresh(np.zeros(3), np.zeros(3), ident, ident, points_gt=gt,
                                                              points_prediction=rec, fscore_threshold=t)
                                             for t in (0.3, 0.9)], np.int64)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays; "
          f"correct_thresh results {out['correct/result'].tolist()}, fscore {out['correct/fscore_result'].tolist()}")


if __name__ == "__main__":
    main()
