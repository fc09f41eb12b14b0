#!/usr/bin/env python3
"""What N orientation hypotheses cost: the time per call of ``SDFPipeline.estimate_hypotheses`` at N = 1 ... 32 beside
``SDFPipeline.__call__`` (one start) and ``SDFPipeline.estimate_objects`` at K = N (N different objects' worth of rows,
here the same mask K times) -- the first measurement of the K-row loop on N IDENTICAL images.

The C5 mug scene of tools/bench_extra.py (640x480, 50 iterations, shape optimisation on) behind a background wall the
mask removes, seeded initialisation-network weights with a plausible final layer.  One process, one pipeline per case
(a pipeline keeps at most ``MAX_CACHED_LOOPS`` loops of a kind).  A sample is `--calls` consecutive calls and a device
synchronisation on the host's clock, divided by `--calls`; every case is built, captured and run twice before anything
is timed; the cases are INTERLEAVED (one sample of each per round, `--repeats` rounds), so a drift of the machine meets
all of them.  Medians and ranges go to profiles/bench_hypotheses.json, with ``ratio_to_1`` = median(N) / median(1) of
``estimate_hypotheses``."""
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


def pipeline(iterations):
    from sdfest_amd import SDFPipeline
    from sdfest_amd.synthetic import MUG_INIT_BACKBONE, MUG_INIT_HEAD, plausible_init_network_state
    gdir = os.path.join(ROOT, "tests", "golden")
    d = np.load(os.path.join(gdir, "decoder_mug.npz"))
    w = np.load(os.path.join(gdir, "mug_decoder_weights.npz"))
    vae = {"latent_size": int(d["latent_size"]), "tsdf": False, "decoder": {
        "fc_layers": [{"out": int(o)} for o in d["fc_out"]],
        "conv_layers": [{"in_size": int(a), "in_channels": int(b), "out_channels": int(c), "kernel_size": int(k),
                         "relu": bool(r)} for a, b, c, k, r in zip(d["conv_in_size"], d["conv_cin"], d["conv_cout"],
                                                                  d["conv_k"], d["conv_relu"])]}}
    cfg = dict(threshold=0.005, max_iterations=iterations, depth_weight=1.0, pc_weight=3.0, device="cuda", nn_weight=0.0,
               mean_shape=False, init_view="first", far_field=2.0,
               camera={"width": 640, "height": 480, "fx": 320.0, "fy": 320.0, "cx": 320.0, "cy": 240.0,
                       "pixel_center": 0.5}, vae=vae,
               init={"backbone_type": "VanillaPointNet", "backbone": dict(MUG_INIT_BACKBONE), "head_type": "SDFPoseHead",
                     "head": dict(MUG_INIT_HEAD), "normalize_pose": True})
    return SDFPipeline(cfg, vae_state_dict={k: w[k] for k in w.files},
                       init_state_dict=plausible_init_network_state(7, scale=0.06))


def sample(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hypotheses", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32])
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--calls", type=int, default=5, help="calls per sample")
    ap.add_argument("--repeats", type=int, default=10, help="interleaved rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_hypotheses.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hypotheses.py measures on the GPU; none found")
    from _loop_scene import c5_scene
    image = c5_scene(views=1, max_iterations=a.iterations)["targets"][0]
    mask = image > 0
    depth = torch.where(mask, image, torch.full_like(image, 1.2)).contiguous()      # a background the mask must remove
    color = torch.zeros((480, 640, 3), device=depth.device)
    arg = torch.empty_like(depth)

    cases = {}
    pipe = pipeline(a.iterations)

    def front_door(pipe=pipe):      # (__call__ masks its argument in place: a fresh copy per call, as a caller makes)
        arg.copy_(depth)
        pipe(arg, mask, color)
    cases["call", 1] = front_door
    for N in a.hypotheses:
        ph, po = pipeline(a.iterations), pipeline(a.iterations)
        masks = mask[None].expand(N, -1, -1).contiguous()
        cases["estimate_hypotheses", N] = lambda ph=ph, N=N: ph.estimate_hypotheses(depth, mask, color, hypotheses=N)
        cases["estimate_objects", N] = lambda po=po, masks=masks: po.estimate_objects(depth, masks)
    for fn in cases.values():      # build, capture, settle
        sample(fn, 1)
        sample(fn, 1)
    times = {k: [] for k in cases}
    for _ in range(a.repeats):
        for k, fn in cases.items():
            times[k].append(sample(fn, a.calls))
    stat = lambda ts: {"median_ms": float(np.median(ts)) * 1e3, "min_ms": float(min(ts)) * 1e3, "max_ms": float(max(ts)) * 1e3}
    results = {"call": stat(times["call", 1]), "estimate_hypotheses": [], "estimate_objects": []}
    base = float(np.median(times["estimate_hypotheses", a.hypotheses[0]]))
    for N in a.hypotheses:
        row = dict(hypotheses=N, **stat(times["estimate_hypotheses", N]))
        row["ratio_to_%d" % a.hypotheses[0]] = float(np.median(times["estimate_hypotheses", N])) / base
        results["estimate_hypotheses"].append(row)
        results["estimate_objects"].append(dict(objects=N, **stat(times["estimate_objects", N])))
        print(f"N={N:2d}: estimate_hypotheses {row['median_ms']:8.3f} ms [{row['min_ms']:.3f}, {row['max_ms']:.3f}] "
              f"({row['ratio_to_%d' % a.hypotheses[0]]:.2f} x N={a.hypotheses[0]}), estimate_objects "
              f"{results['estimate_objects'][-1]['median_ms']:8.3f} ms", flush=True)
    print(f"__call__: {results['call']['median_ms']:.3f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "image": [640, 480], "iterations": a.iterations,
                   "calls_per_sample": a.calls, "repeats": a.repeats, "interleaved": True,
                   "what": "wall clock per call, host clock around calls that end in a device synchronise; "
                           "shape optimisation on; the first two samples of every case are not timed",
                   "results": results}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
