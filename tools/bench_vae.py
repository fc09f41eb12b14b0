"""The VAE on the GPU (sdfest_amd.SDFVAE, csrc/encoder.hip + decoder.hip): milliseconds per call for

  * encode (the mug encoder, means + log_var + z) at N = 1, 16 and 256, with the bytes the launch structure moves
    through HBM and the share of the HBM bound (bytes / 6.3 TB/s, a copy's rate on MI355X) that the time reaches,
  * forward (encode + decode) at N = 16,
  * the reference's benchmark_vae.py pair: inference(n=1), and decode + sum + backward of one latent,
  * as a yardstick, the same encoder written with torch.nn.functional.conv3d / linear on the same GPU.

    python tools/bench_vae.py [--out profiles/bench_vae.json]
    python tools/bench_vae.py --kernel-trace DIR [--out ...]
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HBM_BYTES_PER_S = 6.3e12


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


def mug_vae():
    import encoder_twin as et
    import test_decoder_gpu as D
    from sdfest_amd import SDFVAE
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    w = np.load(os.path.join(GOLDEN, "mug_decoder_weights.npz"))
    g = np.load(os.path.join(GOLDEN, "encoder_mug.npz"))
    state = {k: w[k] for k in w.files}
    state.update({k: g[k] for k in g.files if k.startswith("encoder.")})
    cfg = D.mug_config(d)
    cfg["encoder"] = et.MUG_ENCODER
    return SDFVAE.from_config(cfg, state), state


def hbm_bytes(N):
    """what the launch structure moves per call: the input, conv1's output written and read back, weights, outputs"""
    conv1 = 4 * 31 ** 3 * 4
    return N * (64 ** 3 * 4 + 2 * conv1 + 3 * 8 * 4) + 92280 * 4


def measure(iters):
    import torch
    import torch.nn.functional as F
    from sdfest_amd.synthetic import blobs_sdf
    vae, state = mug_vae()
    out = {"encode": [], "torch_encode": []}
    grid = torch.tensor(blobs_sdf(0)[None, None], device="cuda")
    W = {k: torch.tensor(v, device="cuda") for k, v in state.items() if k.startswith("encoder.")}

    def torch_encoder(x):
        h = x
        for i in (0, 2, 4):
            h = torch.relu(F.conv3d(h, W[f"encoder._features.{i}.weight"], W[f"encoder._features.{i}.bias"], stride=2))
        h = h.flatten(1)
        return (F.linear(h, W["encoder.linear_means.weight"], W["encoder.linear_means.bias"]),
                F.linear(h, W["encoder.linear_log_var.weight"], W["encoder.linear_log_var.bias"]))

    with torch.no_grad():
        for N in (1, 16, 256):
            x = grid.repeat(N, 1, 1, 1, 1).contiguous()
            med, mn = timed(lambda: vae.encode(x, seed=0), iters)
            b = hbm_bytes(N)
            row = {"N": N, "median_ms": med, "min_ms": mn, "hbm_bytes": b,
                   "hbm_bound_ms": round(b / HBM_BYTES_PER_S * 1e3, 4),
                   "share_of_hbm_bound": round(b / HBM_BYTES_PER_S * 1e3 / med, 3)}
            print(json.dumps({"encode": row}), flush=True)
            out["encode"].append(row)
            tm, tmn = timed(lambda: torch_encoder(x), iters)
            m, lv = torch_encoder(x)
            m2, lv2 = vae.encoder(x)
            row = {"N": N, "median_ms": tm, "min_ms": tmn,
                   "max_abs_diff_means": float((m - m2).abs().max()), "speedup": round(tm / med, 2)}
            print(json.dumps({"torch_encode": row}), flush=True)
            out["torch_encode"].append(row)
        x16 = grid.repeat(16, 1, 1, 1, 1).contiguous()
        med, mn = timed(lambda: vae(x16, seed=0), iters)
        out["forward_N16"] = {"median_ms": med, "min_ms": mn}
        med, mn = timed(lambda: vae.inference(n=1, seed=0), iters)
        out["inference_n1"] = {"median_ms": med, "min_ms": mn}
    latent = torch.zeros(8, device="cuda", requires_grad=True)

    def fwd_bwd():
        test = vae.decode(latent.unsqueeze(0))
        torch.sum(test).backward()
    med, mn = timed(fwd_bwd, iters)
    out["decode_sum_backward_n1"] = {"median_ms": med, "min_ms": mn}
    for k in ("forward_N16", "inference_n1", "decode_sum_backward_n1"):
        print(json.dumps({k: out[k]}), flush=True)
    return out


def summarize_trace(trace_dir):
    acc = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name", "")
            m = re.search(r"((?:encoder|normal|clamp|conv|fc|resize)\w*_kernel(?:<[^>]*>)?)", name)
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out")
    ap.add_argument("--kernel-trace", metavar="DIR")
    a = ap.parse_args()
    out = {"timing": "median (and min) of --iters calls, each bracketed by CUDA events; ms",
           "input": "blobs_sdf(0) repeated N times; the mug VAE (tests/golden: encoder_mug.npz, mug_decoder_weights.npz)",
           "hbm_bound": "hbm_bytes / 6.3 TB/s"}
    out.update(measure(a.iters))
    if a.kernel_trace:
        os.makedirs(a.kernel_trace, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.kernel_trace, "--",
               sys.executable, os.path.abspath(__file__), "--iters", "5"]
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
