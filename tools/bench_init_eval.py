#!/usr/bin/env python3
"""Time the initialisation network under eval() on a batch: ``SDFPoseNet.forward_batch`` against the same sets through N
single-set calls, and against the reference's modules restated with torch ops (tests/init_train_twin.py's statement,
fp32, ``training=False``, ``no_grad``) on the same GPU; and one full ``SDFPoseNetTrainer.validate`` over `--batches`
batches including its single host read.

The mug architecture at N = 32 with M = 500 and M = 2500.  Device events around `--iters` calls after `--warmup`; the
sides alternate, `--repeats` times; medians and ranges go to profiles/bench_init_eval.json.  ``--only batch`` (or
``single``, ``torch``) runs one side alone (for a kernel trace).
"""
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
    ap.add_argument("--batches", type=int, default=10, help="batches of the timed validate()")
    ap.add_argument("--only", choices=["batch", "single", "torch"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_init_eval.json"))
    a = ap.parse_args()
    import init_eval_twin as ev
    import init_train_twin as tw
    from sdfest_amd import SDFPoseNetTrainer
    cfg, N = tw.MUG, a.batch
    state = tw.random_state(cfg, 0)
    trainer = SDFPoseNetTrainer(tw.train_config(cfg, batch_size=N), state)
    net = trainer.net()
    params = {k: torch.tensor(state[k], dtype=torch.float32, device="cuda") for k, _ in tw.parameter_shapes(cfg)}
    stats = {f"{p}.{s}": torch.tensor(state[f"{p}.{s}"], dtype=torch.float32, device="cuda")
             for p, _ in tw.stat_shapes(cfg) for s in ("running_mean", "running_var")}
    results = {}
    for M in a.sizes:
        x, t = tw.inputs(cfg, N, M, 0)
        t = ev.targets_with_quaternion(cfg, t, N, 0)
        xd = torch.tensor(x, dtype=torch.float32, device="cuda")
        td = {k: torch.tensor(v, device="cuda") if v.dtype == np.int64 else torch.tensor(v, dtype=torch.float32, device="cuda")
              for k, v in t.items()}
        sets = [xd[n][None] for n in range(N)]

        def batch():
            net.forward_batch(xd)

        def single():
            for s in sets:
                net(s)

        def yardstick():
            with torch.no_grad():
                tw.split(tw.forward(params, cfg, xd, False, stats)[0], cfg)

        sides = {"batch": batch, "single": single, "torch": yardstick}
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
        if not a.only:      # one whole validation pass: host clock around the call, which ends in its one host read
            batches = [(xd, td)] * a.batches
            trainer.validate(batches, "bench")
            torch.cuda.synchronize()
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                trainer.validate(batches, "bench")
                samples.setdefault(f"validate_{a.batches}_batches", []).append((time.perf_counter() - t0) * 1e3)
        results[f"N{N}_M{M}"] = {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
                                for k, v in samples.items()}
        print(f"N={N} M={M}: " + ", ".join(f"{k} {np.median(v):.3f} ms [{min(v):.3f}, {max(v):.3f}]"
                                          for k, v in samples.items()), flush=True)
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "architecture": "mug", "iters": a.iters,
                       "repeats": a.repeats, "results": results}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
