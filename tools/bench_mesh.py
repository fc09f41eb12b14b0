"""Marching cubes on decoded mug grids (sdfest_amd.mesh, csrc/mesh.hip): milliseconds per call for N = 1, 8, 32 grids,
`complete` off and on -- end to end (``SDFPipeline.generate_meshes``: decode + count + read-back + emit), the mesh alone
(``extract_mesh`` on grids already decoded) and the CPU twin (tests/mesh_twin.py, numpy) for comparison.

    python tools/bench_mesh.py [--out profiles/bench_mesh.json]
    python tools/bench_mesh.py --kernel-trace DIR [--out ...]
        the same measurement once more as a child under `rocprofv3 --kernel-trace --stats` (output in DIR), and the
        per-kernel durations grouped by kernel and N (the launch grid's y extent) from its trace
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LEVEL = 0.02
SIZES = (1, 8, 32)


def pipeline():
    import torch
    from sdfest_amd import SDFPipeline
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    w = np.load(os.path.join(GOLDEN, "mug_decoder_weights.npz"))
    vae = {"latent_size": int(d["latent_size"]), "tsdf": False, "decoder": {
        "fc_layers": [{"out": int(o)} for o in d["fc_out"]],
        "conv_layers": [{"in_size": int(a), "in_channels": int(b), "out_channels": int(c), "kernel_size": int(k),
                         "relu": bool(r)} for a, b, c, k, r in zip(d["conv_in_size"], d["conv_cin"], d["conv_cout"],
                                                                  d["conv_k"], d["conv_relu"])]}}
    cfg = {"camera": {"width": 160, "height": 120, "fx": 100.0, "fy": 100.0, "cx": 80.0, "cy": 60.0,
                      "pixel_center": 0.5}, "threshold": 0.005, "device": "cuda", "iso_threshold": LEVEL,
           "max_iterations": 1, "depth_weight": 1.0, "pc_weight": 3.0, "nn_weight": 0.0, "mean_shape": False,
           "init_view": "first", "vae": vae, "init": {"backbone_type": "VanillaPointNet", "head_type": "SDFPoseHead"}}

    def no_init(*args):
        raise RuntimeError("not used")

    pipe = SDFPipeline(cfg, vae_state_dict={k: w[k] for k in w.files}, init_network=no_init)
    z = torch.tensor(d["z"], device="cuda")
    return pipe, z


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
    return statistics.median(out), min(out)


def measure(iters, cpu):
    import torch
    from sdfest_amd import extract_mesh
    import mesh_twin
    pipe, z12 = pipeline()
    tabs = mesh_twin.tables()
    res = []
    for N in SIZES:
        z = z12[torch.arange(N) % z12.shape[0]].contiguous()
        scales = torch.full((N,), 0.1, device="cuda")
        grids = pipe.vae.decode(z)[:, 0].contiguous()
        host = grids.cpu().numpy()
        for complete in (False, True):
            e2e = timed(lambda: pipe.generate_meshes(z, scales, complete_mesh=complete), iters)
            mesh = timed(lambda: extract_mesh(grids, LEVEL, complete=complete), iters)
            dec = timed(lambda: pipe.vae.decode(z), iters)
            ms = extract_mesh(grids, LEVEL, complete=complete)
            row = {"N": N, "complete": complete, "generate_meshes_ms": round(e2e[0], 3),
                   "generate_meshes_min_ms": round(e2e[1], 3), "extract_mesh_ms": round(mesh[0], 3),
                   "extract_mesh_min_ms": round(mesh[1], 3), "decode_ms": round(dec[0], 3),
                   "vertices": int(sum(m.vertices.shape[0] for m in ms)),
                   "faces": int(sum(m.faces.shape[0] for m in ms))}
            if cpu:
                t0 = time.perf_counter()
                for n in range(N):
                    mesh_twin.marching_cubes(host[n], LEVEL, complete=complete, tabs=tabs)
                row["cpu_twin_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            print(json.dumps(row), flush=True)
            res.append(row)
    return res


def summarize_trace(trace_dir):
    acc = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name", "")
            m = re.search(r"(mesh_\w+_kernel)", name)
            if not m:
                continue
            gy = int(r.get("Grid_Size_Y", r.get("Grid_Y", 0)) or 0)
            wy = int(r.get("Workgroup_Size_Y", r.get("Workgroup_Y", 1)) or 1)
            gx = int(r.get("Grid_Size_X", r.get("Grid_X", 0)) or 0)
            key = (m.group(1), gy // max(wy, 1), gx)
            acc.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    rows = []
    for (k, gy, gx), v in sorted(acc.items(), key=lambda kv: (kv[0][2], kv[0][1], kv[0][0])):
        rows.append({"kernel": k, "grid_y": gy, "grid_x_threads": gx, "calls": len(v),
                     "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--kernel-trace", metavar="DIR")
    a = ap.parse_args()
    out = {"level": LEVEL, "grid": "64^3 decoded mug latents (tests/golden/decoder_mug.npz z, cycled)",
           "timing": "median of --iters calls, each synchronised; ms"}
    out["calls"] = measure(a.iters, not a.no_cpu)
    if a.kernel_trace:
        os.makedirs(a.kernel_trace, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.kernel_trace, "--",
               sys.executable, os.path.abspath(__file__), "--iters", "10", "--no-cpu"]
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
