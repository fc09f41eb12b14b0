"""Surface sampling and reconstruction metrics on the GPU (sdfest_amd.metrics, Mesh.sample_points_uniformly,
csrc/metrics.hip): milliseconds per call for

  * sampling 20 000 points on 1, 8 and 32 mug meshes (sample_points, one launch sequence),
  * one nearest pass (p = 2, sdfr_nn_query) at 20 000 x 20 000, 100 000 x 100 000 and K = 32 pairs of 20 000 x 20 000,
  * the full rendering_evaluation.yaml metric set per object (evaluate_metrics on 20 000-point sets), and the same
    after sampling both meshes (mesh -> score),
  * scipy's KDTree doing the reference's calls for the same metric set (one tree build + query per metric, as
    sdfest/estimation/metrics.py does), on this process's CPU share, where scipy is installed.

    python tools/bench_metrics.py [--out profiles/bench_metrics.json]
    python tools/bench_metrics.py --kernel-trace DIR [--out ...]
        the same measurement once more as a child under `rocprofv3 --kernel-trace --stats` (output in DIR), and the
        per-kernel durations grouped by kernel and launch grid from its trace
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
N_SAMPLES = 20000
RENDERING_EVALUATION = {
    "mean_accuracy": {"f": "sdfest.estimation.metrics.mean_accuracy", "kwargs": {}},
    "mean_completeness": {"f": "sdfest.estimation.metrics.mean_completeness", "kwargs": {}},
    "chamfer": {"f": "sdfest.estimation.metrics.symmetric_chamfer", "kwargs": {}},
    "completeness_0_01": {"f": "sdfest.estimation.metrics.completeness_thresh", "kwargs": {"threshold": 0.01}},
    "accuracy_0_01": {"f": "sdfest.estimation.metrics.accuracy_thresh", "kwargs": {"threshold": 0.01}},
}


def timed(fn, iters, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out), 4), round(min(out), 4)


def mug_meshes():
    import torch
    from sdfest_amd import Mesh, extract_mesh
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    m = extract_mesh(torch.tensor(d["z0_full"], device="cuda"), 0.02, complete=True)
    gt = Mesh(m.vertices, m.faces, scale=0.1, rel_scale=True, orientation=[0.0, 0.0, 0.0, 1.0], position=[0, 0, 0.7])
    est = Mesh(m.vertices * 1.02, m.faces, scale=0.1, rel_scale=True,
               orientation=[0.0, 0.0, 0.0998, 0.995], position=[0.003, 0.0, 0.7])
    return gt, est


def scipy_rendering_evaluation(gt, rec):
    """the five metrics the way the reference computes them: a KDTree built and queried per call"""
    import scipy.spatial

    def query(a, b):
        return scipy.spatial.KDTree(a).query(b, p=2)[0]

    acc = np.mean(query(gt, rec))
    comp = np.mean(query(rec, gt))
    chamfer = (np.mean(query(rec, gt)) + np.mean(query(gt, rec))) / 2
    c01 = np.sum(query(rec, gt) < 0.01) / gt.shape[0]
    a01 = np.sum(query(gt, rec) < 0.01) / rec.shape[0]
    return {"mean_accuracy": acc, "mean_completeness": comp, "chamfer": chamfer, "completeness_0_01": c01,
            "accuracy_0_01": a01}


def measure(iters, cpu):
    import torch
    from sdfest_amd import evaluate_metrics, sample_points
    from sdfest_amd.metrics import _nn, _pack, _points
    gt_mesh, est_mesh = mug_meshes()
    out = {"sampling": [], "nearest_pass": [], "evaluation": []}
    for K in (1, 8, 32):
        ms = [gt_mesh if k % 2 == 0 else est_mesh for k in range(K)]
        t = timed(lambda: sample_points(ms, N_SAMPLES, seed=0), iters)
        row = {"meshes": K, "points": N_SAMPLES, "faces_per_mesh": int(gt_mesh.faces.shape[0]), "ms": t[0],
               "min_ms": t[1]}
        print(json.dumps(row), flush=True)
        out["sampling"].append(row)
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    for K, n in ((1, 20000), (1, 100000), (32, 20000)):
        sets = [_points(rng.normal(size=(n, 3)).astype(np.float32) * 0.1, dev, "q") for _ in range(K)]
        refs = [_points(rng.normal(size=(n, 3)).astype(np.float32) * 0.1, dev, "r") for _ in range(K)]
        qp, qoff, qs = _pack(sets, dev)
        rp, roff, rs = _pack(refs, dev)
        t = timed(lambda: _nn(qp, qoff, qs, rp, roff, rs, 2.0, False, dev), iters)
        pairs = K * n * n
        row = {"pairs_K": K, "queries": n, "refs": n, "ms": t[0], "min_ms": t[1],
               "pairs_per_s": float(f"{pairs / (t[1] * 1e-3):.4g}")}
        print(json.dumps(row), flush=True)
        out["nearest_pass"].append(row)
    a = gt_mesh.sample_points_uniformly(N_SAMPLES, seed=0)
    b = est_mesh.sample_points_uniformly(N_SAMPLES, seed=0)
    t = timed(lambda: evaluate_metrics(a, b, RENDERING_EVALUATION), iters)
    t2 = timed(lambda: evaluate_metrics(gt_mesh.sample_points_uniformly(N_SAMPLES, seed=0),
                                        est_mesh.sample_points_uniformly(N_SAMPLES, seed=0), RENDERING_EVALUATION),
               iters)
    gpu_vals = evaluate_metrics(a, b, RENDERING_EVALUATION)
    row = {"what": "rendering_evaluation.yaml metric set, 20000 vs 20000 points", "evaluate_metrics_ms": t[0],
           "evaluate_metrics_min_ms": t[1], "sample_and_evaluate_ms": t2[0], "values": gpu_vals}
    if cpu:
        try:
            import scipy  # noqa: F401
            an, bn = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            ref_vals = scipy_rendering_evaluation(an, bn)
            row["scipy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["scipy_values"] = {k: float(v) for k, v in ref_vals.items()}
            row["cpu_threads"] = len(os.sched_getaffinity(0))
        except ImportError:
            row["scipy_ms"] = None
            row["scipy_note"] = "scipy is not installed here: no CPU comparison"
    print(json.dumps(row), flush=True)
    out["evaluation"].append(row)
    return out


def summarize_trace(trace_dir):
    acc = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name", "")
            m = re.search(r"((?:sample|nn)\w*_kernel(?:<[^>]*>)?)", name)
            if not m:
                continue
            grid = tuple(int(r.get(f"Grid_Size_{a}", r.get(f"Grid_{a}", 0)) or 0) for a in "XYZ")
            acc.setdefault((m.group(1), grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    rows = []
    for (k, grid), v in sorted(acc.items()):
        rows.append({"kernel": k, "grid_threads_xyz": list(grid), "calls": len(v),
                     "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--kernel-trace", metavar="DIR")
    a = ap.parse_args()
    out = {"timing": "median (and min) of --iters calls, each synchronised; ms",
           "meshes": "the decoded mug (tests/golden/decoder_mug.npz z0_full, level 0.02, complete) at scale 0.1, "
                     "ground truth and a perturbed, rotated estimate",
           "points": "nearest_pass: normal(0, 0.1) float32 sets"}
    out.update(measure(a.iters, not a.no_cpu))
    if a.kernel_trace:
        os.makedirs(a.kernel_trace, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.kernel_trace, "--",
               sys.executable, os.path.abspath(__file__), "--iters", "5", "--no-cpu"]
        rc = subprocess.run(cmd, timeout=600).returncode
        out["kernel_trace_rc"] = rc
        out["kernels"] = summarize_trace(a.kernel_trace)
        for r in out["kernels"]:
            print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
