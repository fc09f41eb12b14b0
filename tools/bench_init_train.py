#!/usr/bin/env python3
"""Time one training iteration of the initialisation network: ``SDFPoseNetTrainer.step`` against the same iteration
written with torch ops under autograd + ``torch.optim.Adam`` (tests/init_train_twin.py's statement, fp32) on the same GPU.

The mug architecture at N = 32 with M = 500 and M = 2500.  Device events around `--iters` iterations after `--warmup`;
the two sides alternate, `--repeats` times; medians and ranges go to profiles/bench_init_train.json.  ``--only ours``
runs the trainer alone (for a kernel trace).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 2500])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["ours", "torch"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_init_train.json"))
    a = ap.parse_args()
    import init_train_twin as tw
    from sdfest_amd import SDFPoseNetTrainer
    cfg, N = tw.MUG, a.batch
    state = tw.random_state(cfg, 0)
    results = {}
    for M in a.sizes:
        x, t = tw.inputs(cfg, N, M, 0)
        xd = torch.tensor(x, dtype=torch.float32, device="cuda")
        td = {k: torch.tensor(v, device="cuda") if v.dtype == np.int64 else torch.tensor(v, dtype=torch.float32, device="cuda")
              for k, v in t.items()}
        trainer = SDFPoseNetTrainer(tw.train_config(cfg), state)
        params = {k: torch.tensor(state[k], dtype=torch.float32, device="cuda", requires_grad=True)
                  for k, _ in tw.parameter_shapes(cfg)}
        stats = {f"{p}.{s}": torch.tensor(state[f"{p}.{s}"], dtype=torch.float32, device="cuda")
                 for p, _ in tw.stat_shapes(cfg) for s in ("running_mean", "running_var")}
        opt = torch.optim.Adam(list(params.values()), lr=1e-3)

        def ours():
            trainer.step(xd, td)

        def yardstick():
            opt.zero_grad()
            out, new = tw.forward(params, cfg, xd, True, stats)
            tw.loss(out, td, cfg)["total"].backward()
            opt.step()
            stats.update(new)

        sides = {"ours": ours, "torch": yardstick}
        if a.only:
            sides = {a.only: sides[a.only]}
        for fn in sides.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in sides}
        for _ in range(a.repeats):
            for k, fn in sides.items():
                samples[k].append(timed(fn, a.iters))
        results[f"N{N}_M{M}"] = {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
                                for k, v in samples.items()}
        print(f"N={N} M={M}: " + ", ".join(f"{k} {np.median(v):.3f} ms [{min(v):.3f}, {max(v):.3f}]"
                                          for k, v in samples.items()), flush=True)
        del trainer, params, opt
        torch.cuda.empty_cache()
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "architecture": "mug", "iters": a.iters,
                       "repeats": a.repeats, "results": results}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
