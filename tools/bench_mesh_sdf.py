"""Mesh -> SDF volume (sdfest_amd.mesh_to_sdf, csrc/mesh_sdf.hip): milliseconds per synchronised call and
point-triangle pairs per second.

Cases: the mug's marching-cubes mesh (about 37 k faces) at R = 64 as one mesh and as a batch of 8, signed and unsigned
(their difference is the cost of the winding half); the same mesh at R = 32; the 204 160-face sphere of
tools/bench_mesh_depth.py at R = 64.  Nothing on the CPU or in the reference to time against (its mesh_to_sdf package
is not installed).  After a warm-up of every case the cases are timed interleaved, `--repeats` rounds of `--iters`
calls; the figure is the median over all of a case's calls.

    python tools/bench_mesh_sdf.py [--out profiles/bench_mesh_sdf.json]
    python tools/bench_mesh_sdf.py --kernel-trace DIR [--out ...]
        the same calls once more as a child under `rocprofv3 --kernel-trace --stats` (output in DIR), and the
        per-kernel durations from its trace, grouped by kernel and grid
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cases():
    import torch
    import raster_twin as rt
    from bench_mesh import pipeline
    from sdfest_amd import Mesh, mesh_to_sdf
    dev = "cuda"
    T = lambda a, dt=torch.float32: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    pipe, z = pipeline()
    mug = pipe.generate_mesh(z[9:10] * 0.5, T([1.0]), True)
    v, f = rt.uv_sphere(320, 320, 1.0)
    fine = Mesh(T(v), T(f, torch.int32), scale=0.5, rel_scale=True)
    out = {}

    def add(name, mesh, K, R, signed):
        meshes = [mesh] * K if K > 1 else mesh
        buf = torch.empty((K, R, R, R) if K > 1 else (R, R, R), device=dev)
        out[name] = (lambda: mesh_to_sdf(meshes, R, padding=2, signed=signed, out=buf), int(mesh.faces.shape[0]), K, R,
                     signed)

    add("mug_r64_signed", mug, 1, 64, True)
    add("mug_r64_unsigned", mug, 1, 64, False)
    add("mug_r64_k8_signed", mug, 8, 64, True)
    add("mug_r64_k8_unsigned", mug, 8, 64, False)
    add("mug_r32_signed", mug, 1, 32, True)
    add("fine_sphere_r64_signed", fine, 1, 64, True)
    return out


def measure(iters, repeats):
    import torch
    cs = cases()
    with torch.no_grad():
        for fn, *_ in cs.values():       # warm-up: every shape the timed window uses
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in cs}
        inside = {}
        for _ in range(repeats):
            for name, (fn, *_) in cs.items():
                for _ in range(iters):
                    t0 = time.perf_counter()
                    vol = fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) * 1e3)
                inside[name] = float((vol < 0).float().mean())
    rows = []
    for name, (_, faces, K, R, signed) in cs.items():
        ms = statistics.median(times[name])
        pairs = K * R ** 3 * faces
        row = {"case": name, "faces": faces, "meshes": K, "R": R, "signed": signed, "ms": round(ms, 4),
               "min_ms": round(min(times[name]), 4), "pairs": pairs, "gpairs_per_s": round(pairs / ms / 1e6, 2),
               "negative_share": round(inside[name], 4)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def summarize_trace(trace_dir):
    acc = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"(mesh_sdf_\w*kernel(?:<\w+>)?)", r.get("Kernel_Name", ""))
            if not m:
                continue
            grid = tuple(int(r.get(f"Grid_Size_{a}", 0) or 0) for a in "XYZ")
            acc.setdefault((m.group(1), grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return [{"kernel": k, "grid_threads": list(g), "calls": len(v), "median_us": round(statistics.median(v), 2),
             "min_us": round(min(v), 2)} for (k, g), v in sorted(acc.items(), key=lambda kv: (kv[0][0], kv[0][1]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--out")
    ap.add_argument("--kernel-trace", metavar="DIR")
    a = ap.parse_args()
    out = {"timing": "median over --repeats interleaved rounds of --iters calls, each synchronised; ms; a pair is one "
                     "grid point against one face"}
    out["calls"] = measure(a.iters, a.repeats)
    if a.kernel_trace:
        os.makedirs(a.kernel_trace, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.kernel_trace, "--",
               sys.executable, os.path.abspath(__file__), "--iters", "2", "--repeats", "1"]
        out["kernel_trace_rc"] = subprocess.run(cmd, timeout=600).returncode
        out["kernels"] = summarize_trace(a.kernel_trace)
        for r in out["kernels"]:
            print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
