"""Training of the VAE on the GPU (sdfest_amd.SDFVAETrainer, csrc/vae_train.hip): milliseconds per ``step`` (forward,
loss, backward, Adam) for the mug config at batch 8 (the reference's default) and batch 64, and as a yardstick the same
iteration written with torch ops under autograd plus torch.optim.Adam on the same GPU.  ``step_pc``: the same step with
the point cloud term (pc_weight = 1: a 640 x 480 render of every target and ``sdfr_vae_trainer_pc_term``) against
pc_weight = 0 in the same process, the two trainers taking turns (--rounds blocks of --iters steps each).

    python tools/bench_vae_train.py [--out profiles/bench_vae_train.json]
    python tools/bench_vae_train.py --kernel-trace DIR [--stats-out profiles/bench_vae_train_kernel_stats.csv] [--out ...]
        the trainer's steps at batch 8 once more as a child under `rocprofv3 --kernel-trace --stats` (output in DIR); its
        per-kernel statistics are copied to --stats-out
"""
import argparse
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, iters, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return round(statistics.median(ts), 4), round(min(ts), 4)


def setup(N):
    import torch
    import vae_train_twin as tw
    from sdfest_amd.synthetic import blobs_sdf
    config, state = tw.mug_setup()
    config = dict(config, warm_up_iterations=0, batch_size=N)     # the post phase: clamp, mask and KLD all live
    x = torch.tensor(np.stack([blobs_sdf(s % 4) for s in range(N)])[:, None], device="cuda")
    return config, state, x


def measure_pc(iters, N, rounds):
    """pc_weight 0 and 1, interleaved: [median ms of each block] per weight, and the allocator's calls per step"""
    import torch
    from sdfest_amd import SDFVAETrainer
    config, state, x = setup(N)
    trainers = {w: SDFVAETrainer(dict(config, pc_weight=w), state) for w in (0.0, 1.0)}
    blocks = {w: [] for w in trainers}
    for t in trainers.values():
        t.iteration = 1
    for _ in range(rounds):
        for w, t in trainers.items():
            blocks[w].append(timed(lambda: t.step(x, seed=1), iters)[0])
    allocs = {}
    for w, t in trainers.items():     # after the first calls at this batch size: what one more step asks the allocator for
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        t.step(x, seed=1)
        allocs[w] = torch.cuda.memory_stats()["allocation.all.allocated"] - before
    torch.cuda.synchronize()
    m0, m1 = statistics.median(blocks[0.0]), statistics.median(blocks[1.0])
    return {"N": N, "pc_weight_0_ms": blocks[0.0], "pc_weight_1_ms": blocks[1.0], "median_0_ms": round(m0, 4),
            "median_1_ms": round(m1, 4), "term_ms": round(m1 - m0, 4), "allocations_per_step": [allocs[0.0], allocs[1.0]]}


def measure(iters, batches, with_torch=True, rounds=3):
    import torch
    import vae_train_twin as tw
    from sdfest_amd import SDFVAETrainer
    out = {"step": [], "torch_step": [], "step_pc": []}
    for N in batches:
        row = measure_pc(iters, N, rounds)
        print(json.dumps({"step_pc": row}), flush=True)
        out["step_pc"].append(row)
        config, state, x = setup(N)
        t = SDFVAETrainer(config, state)
        t.iteration = 1
        med, mn = timed(lambda: t.step(x, seed=1), iters)
        row = {"N": N, "median_ms": med, "min_ms": mn}
        print(json.dumps({"step": row}), flush=True)
        out["step"].append(row)
        if not with_torch:
            continue
        params = {k: torch.tensor(v, device="cuda", requires_grad=True) for k, v in state.items()}
        opt = torch.optim.Adam(list(params.values()), lr=config["learning_rate"])
        eps = torch.randn(N, config["latent_size"], device="cuda")

        def torch_step():
            xc = x.clamp(-config["tsdf"], config["tsdf"])
            means, log_var, _, recon = tw.forward(params, config, xc, eps)
            terms = tw.loss(recon, xc, means, log_var, config, True)
            opt.zero_grad()
            terms["total"].backward()
            opt.step()
        tm, tmn = timed(torch_step, iters)
        row = {"N": N, "median_ms": tm, "min_ms": tmn, "torch_over_trainer": round(tm / med, 3)}
        print(json.dumps({"torch_step": row}), flush=True)
        out["torch_step"].append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--rounds", type=int, default=3, help="blocks per weight of the interleaved pc_weight 0 / 1 rows")
    ap.add_argument("--trainer-only", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--kernel-trace", metavar="DIR")
    ap.add_argument("--stats-out")
    a = ap.parse_args()
    out = {"timing": "median (and min) of --iters steps, each bracketed by device events; ms",
           "workload": "the mug VAE (tests/golden), blobs_sdf volumes, post phase (tsdf 0.1, all five loss terms live); "
                       "step = forward + loss + backward + Adam; torch_step = the same iteration with torch ops under "
                       "autograd + torch.optim.Adam on the same GPU"}
    out["workload"] += ("; step_pc = step with pc_weight 0 and 1 (the reference's 640 x 480 camera), two trainers taking "
                        "turns in one process, median ms of each block of --iters steps")
    out.update(measure(a.iters, a.batches, not a.trainer_only, a.rounds))
    if a.kernel_trace:
        os.makedirs(a.kernel_trace, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.kernel_trace, "--",
               sys.executable, os.path.abspath(__file__), "--iters", "10", "--batches", "8", "--trainer-only", "--rounds", "1"]
        out["kernel_trace_rc"] = subprocess.run(cmd, timeout=600).returncode
        stats = glob.glob(os.path.join(a.kernel_trace, "**", "*kernel_stats.csv"), recursive=True)
        if stats and a.stats_out:
            shutil.copyfile(stats[0], a.stats_out)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
