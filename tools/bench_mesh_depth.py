"""The mesh depth rasteriser (sdfest_amd.render_mesh_depth, csrc/raster.hip): milliseconds per synchronised call, and
beside each the time ``render_depth_batch`` (the sphere tracer) takes for the same object, pose count and image size
-- the scale to read it against.

Cases, all 640 x 480, f = 320: one view of the mug's marching-cubes mesh; 256 seeded poses of it in one call; one
view of a sphere of 204 160 sub-pixel triangles (against the tracer on ``sphere_sdf``); one view of a cube of 12
triangles that fills the image (no tracer counterpart).  After a warm-up of every case the cases are timed
interleaved, `--repeats` rounds of `--iters` calls; the figure is the median over all of a case's calls.

    python tools/bench_mesh_depth.py [--out profiles/bench_mesh_depth.json]
    python tools/bench_mesh_depth.py --kernel-trace DIR [--out ...]
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
W, H, F_PIX, THRESHOLD = 640, 480, 320.0, 0.005


def cases():
    import torch
    import raster_twin as rt
    from bench_mesh import pipeline
    from sdfest_amd import Camera, Mesh, render_depth_batch, render_mesh_depth
    from sdfest_amd.synthetic import random_poses, sphere_sdf
    dev = "cuda"
    T = lambda a, dt=torch.float32: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    cam = Camera(W, H, F_PIX, F_PIX, W / 2, H / 2, pixel_center=0.5)
    pipe, z = pipeline()
    z1 = z[9:10] * 0.5
    with torch.no_grad():
        mug_sdf = pipe.vae.decode(z1)[0, 0].contiguous()
    mug = pipe.generate_mesh(z1, T([1.0]), True)
    q1 = T([[0.2, 0.6, -0.15, 0.75]])
    q1 = q1 / q1.norm()
    p1, s1 = T([[0.02, -0.01, -0.5]]), 0.055
    pos, quat, inv_scale = (T(a) for a in random_poses(256, seed=1, width=W, height=H, f=F_PIX))
    v, f = rt.uv_sphere(320, 320, 1.0)
    fine = Mesh(T(v), T(f, torch.int32), scale=0.5, rel_scale=True)
    ball_sdf = T(sphere_sdf(0.5, 64))
    cv, cf = rt.cube(1.0)
    cube = Mesh(T(cv), T(cf, torch.int32), scale=0.3, rel_scale=True)
    cube_q = T([[0.03, -0.04, 0.02, 1.0]])
    cube_q = cube_q / cube_q.norm()
    out = {}

    def mesh_call(mesh, scale, p, q):
        buf = torch.empty((p.shape[0], H, W), device=dev)

        def call():
            mesh.update_scale(scale, rel_scale=True)
            return render_mesh_depth(mesh, cam, p, q, out=buf)
        return call

    def tracer_call(sdf, scale, p, q):
        isc = torch.full((p.shape[0],), 1.0 / scale, device=dev)
        return lambda: render_depth_batch(sdf, p, q, isc, THRESHOLD, cam)

    out["mug_1_view"] = (mesh_call(mug, s1, p1, q1), tracer_call(mug_sdf, s1, p1, q1), int(mug.faces.shape[0]), 1)
    # the 256 poses of synthetic.random_poses with one scale (a mesh has one scale): the mean of theirs
    sc = float((1.0 / inv_scale).mean())
    out["mug_256_poses"] = (mesh_call(mug, sc, pos, quat), tracer_call(mug_sdf, sc, pos, quat),
                            int(mug.faces.shape[0]), 256)
    out["fine_sphere_1_view"] = (mesh_call(fine, 0.2, p1, q1), tracer_call(ball_sdf, 0.2 * 2, p1, q1),
                                 int(fine.faces.shape[0]), 1)
    out["cube_fills_image"] = (mesh_call(cube, 0.3, T([[0.01, -0.02, -0.62]]), cube_q), None, 12, 1)
    return out


def measure(iters, repeats):
    import torch
    cs = cases()
    with torch.no_grad():
        for mesh_fn, tracer_fn, _, _ in cs.values():       # warm-up: every shape the timed window uses
            for _ in range(3):
                mesh_fn()
                if tracer_fn is not None:
                    tracer_fn()
        torch.cuda.synchronize()
        times = {name: ([], []) for name in cs}
        hits = {}
        for _ in range(repeats):
            for name, (mesh_fn, tracer_fn, _, _) in cs.items():
                for which, fn in enumerate((mesh_fn, tracer_fn)):
                    if fn is None:
                        continue
                    for _ in range(iters):
                        t0 = time.perf_counter()
                        img = fn()
                        torch.cuda.synchronize()
                        times[name][which].append((time.perf_counter() - t0) * 1e3)
                    hits.setdefault(name, [None, None])[which] = float((img > 0).float().mean())
    rows = []
    for name, (_, tracer_fn, faces, views) in cs.items():
        m, t = times[name]
        row = {"case": name, "faces": faces, "views": views, "mesh_depth_ms": round(statistics.median(m), 4),
               "mesh_depth_min_ms": round(min(m), 4), "hit_share": round(hits[name][0], 4)}
        if tracer_fn is not None:
            row.update({"render_depth_batch_ms": round(statistics.median(t), 4),
                        "render_depth_batch_min_ms": round(min(t), 4), "tracer_hit_share": round(hits[name][1], 4)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def summarize_trace(trace_dir):
    acc = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"(raster_\w+_kernel|render_forward\w*)", r.get("Kernel_Name", ""))
            if not m:
                continue
            grid = tuple(int(r.get(f"Grid_Size_{a}", 0) or 0) for a in "XYZ")
            acc.setdefault((m.group(1), grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return [{"kernel": k, "grid_threads": list(g), "calls": len(v), "median_us": round(statistics.median(v), 2),
             "min_us": round(min(v), 2)} for (k, g), v in sorted(acc.items(), key=lambda kv: (kv[0][0], kv[0][1]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--kernel-trace", metavar="DIR")
    a = ap.parse_args()
    out = {"image": [W, H], "f": F_PIX, "tracer_threshold": THRESHOLD,
           "timing": "median over --repeats interleaved rounds of --iters calls, each synchronised; ms"}
    out["calls"] = measure(a.iters, a.repeats)
    if a.kernel_trace:
        os.makedirs(a.kernel_trace, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.kernel_trace, "--",
               sys.executable, os.path.abspath(__file__), "--iters", "3", "--repeats", "2"]
        out["kernel_trace_rc"] = subprocess.run(cmd, timeout=600).returncode
        out["kernels"] = summarize_trace(a.kernel_trace)
        for r in out["kernels"]:
            print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
