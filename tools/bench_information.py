#!/usr/bin/env python3
"""What the pose information costs: ``sdfr_render_information`` on the benchmark's inputs beside ``sdfr_render_backward``
on the same inputs, and ``SDFPipeline.pose_uncertainty()`` beside the front-door call it follows.

Part 1: 256 views of 640x480 of blobs(0) at ``synthetic.random_poses`` (bench.py's inputs), threshold 0.005; the estimate
is the forward at those poses, the target the forward at slightly moved poses (position + (0.01, -0.008, 0.012), scale
/ 1.03).  ``render_information(depth, target, ...)`` against ``backward_raw(depth - target, depth, ...)``: the same
gathers per hit pixel, one without and one with a gradient volume to write.  A sample is `--calls` consecutive calls
between two device events; both are warmed up and the samples INTERLEAVED (`--repeats` rounds).
Part 2: the C5 mug scene of tools/bench_hypotheses.py through ``SDFPipeline.__call__`` (pose and shape, `--iterations`
iterations), then ``pose_uncertainty()``: host clock around calls that end in a device synchronise.
Medians and ranges go to profiles/bench_information.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def event_sample(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def host_sample(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def stat(ts, unit):
    k = {"us": 1e6, "ms": 1e3}[unit]
    return {f"median_{unit}": float(np.median(ts)) * k, f"min_{unit}": float(min(ts)) * k, f"max_{unit}": float(max(ts)) * k}


def kernel_part(a):
    from sdfest_amd import Camera, render_information
    from sdfest_amd.differentiable_renderer import backward_raw, forward_raw
    from sdfest_amd.synthetic import blobs_sdf, random_poses
    W, H, B, thr = 640, 480, a.views, 0.005
    dev = torch.device("cuda:0")
    t = lambda x: torch.tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)
    sdf = t(blobs_sdf(0))
    pos, quat, isc = (t(x) for x in random_poses(B, seed=1, width=W, height=H, f=W / 2.0))
    cam = Camera(W, H, W / 2.0, W / 2.0, W / 2.0, H / 2.0, pixel_center=0.5)
    args = (W, H, W / 2.0, H / 2.0, W / 2.0, W / 2.0)
    depth = forward_raw(sdf, pos, quat, isc, *args, thr)
    target = forward_raw(sdf, pos + t([0.01, -0.008, 0.012]), quat, isc * 1.03, *args, thr)
    upstream = ((depth - target) * ((depth > 0) & (target > 0))).contiguous()
    cases = {"render_information": lambda: render_information(depth, target, sdf, pos, quat, isc, cam),
             "render_information_inliers_0.03": lambda: render_information(depth, target, sdf, pos, quat, isc, cam, 0.03),
             "render_backward": lambda: backward_raw(upstream, depth, sdf, pos, quat, isc, *args)}
    gram = cases["render_information"]()
    g_pos, g_quat, g_isc = backward_raw(upstream, depth, sdf, pos, quat, isc, *args)[1:]
    jtr = torch.cat([g_pos, g_quat, g_isc[:, None]], 1).double()
    scale = gram[:, :8, 8].abs().max().item()
    agree = ((gram[:, :8, 8] - jtr).abs().max().item()) / scale      # faster and different is not faster
    for fn in cases.values():
        event_sample(fn, 3)
        event_sample(fn, 3)
    times = {k: [] for k in cases}
    for _ in range(a.repeats):
        for k, fn in cases.items():
            times[k].append(event_sample(fn, a.calls))
    out = {k: stat(v, "us") for k, v in times.items()}
    out["information_over_backward"] = float(np.median(times["render_information"]) / np.median(times["render_backward"]))
    out["hit_pixels"] = int((depth > 0).sum().item())
    out["included_pixels"] = int(gram[:, 9, 9].sum().item())
    out["max_abs_J^T_r_minus_backward_over_max"] = agree
    for k in cases:
        print(f"{k:34s} {out[k]['median_us']:9.1f} us [{out[k]['min_us']:.1f}, {out[k]['max_us']:.1f}]", flush=True)
    print(f"information / backward = {out['information_over_backward']:.2f}; J^T r vs the backward: {agree:.2e} of its maximum",
          flush=True)
    return out


def pipeline_part(a):
    from _loop_scene import c5_scene
    from bench_hypotheses import pipeline
    pipe = pipeline(a.iterations)
    image = c5_scene(views=1, max_iterations=a.iterations)["targets"][0]
    mask = image > 0
    depth = torch.where(mask, image, torch.full_like(image, 1.2)).contiguous()
    color = torch.zeros((480, 640, 3), device=depth.device)
    arg = torch.empty_like(depth)

    def front_door():
        arg.copy_(depth)
        pipe(arg, mask, color)
    cases = {"call": front_door, "pose_uncertainty": pipe.pose_uncertainty}
    for fn in cases.values():
        host_sample(fn, 1)
        host_sample(fn, 1)
    times = {k: [] for k in cases}
    for _ in range(a.repeats):
        for k, fn in cases.items():
            times[k].append(host_sample(fn, max(1, a.calls // 4)))
    out = {k: stat(v, "ms") for k, v in times.items()}
    rec = pipe.pose_uncertainty()
    out["rank"] = int(rec.rank[0])
    out["position_std_m"] = rec.position_std[0].tolist()
    out["rotation_std_deg"] = rec.rotation_std_deg[0].tolist()
    for k in cases:
        print(f"{k:34s} {out[k]['median_ms']:9.3f} ms [{out[k]['min_ms']:.3f}, {out[k]['max_ms']:.3f}]", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--calls", type=int, default=20, help="calls per sample")
    ap.add_argument("--repeats", type=int, default=15, help="interleaved rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_information.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_information.py measures on the GPU; none found")
    results = {"kernel": kernel_part(a), "pipeline": pipeline_part(a)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "image": [640, 480], "views": a.views,
                   "iterations": a.iterations, "calls_per_sample": a.calls, "repeats": a.repeats, "interleaved": True,
                   "what": "kernel: device events around calls_per_sample calls, us per call (both launches of "
                           "render_information; prologue, image kernel and reduce of render_backward, plus the "
                           "wrappers' allocations); pipeline: host clock around calls that end in a device synchronise; "
                           "the first two samples of every case are not timed",
                   "results": results}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
