#!/usr/bin/env python3
"""What the shape uncertainty costs, in three pairs (the method of tools/bench_information.py: warmed up, samples
INTERLEAVED over `--repeats` rounds, a sample being `--calls` consecutive calls between two device events).

Part 1, decoder: ``sdfr_decoder_jvp`` of the mug decoder at N = 1 with the identity basis (T = 8, the C call alone on a
tape made beforehand) beside ``sdfr_decoder_forward`` of 8 latents (the batch a JVP's rows amount to), and
``SDFDecoder.jvp`` whole (taped forward + JVP + its allocations).
Part 2, kernel: ``sdfr_render_information_shape`` at T = 8 beside ``sdfr_render_information`` on the same 256 views of
640x480 of blobs(0) (tools/bench_information.py's inputs); the Jacobian is a random (64^3, 8) buffer -- the gathers do
not depend on what it holds.
Part 3, pipeline: ``SDFPipeline.shape_uncertainty()`` beside ``pose_uncertainty()`` after a front-door call on the C5 mug
scene: host clock around calls that end in a device synchronise.
Medians and ranges go to profiles/bench_shape_information.json."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from bench_information import event_sample, host_sample, stat  # noqa: E402


def interleaved(cases, sample, calls, repeats):
    for fn in cases.values():
        sample(fn, 3)
        sample(fn, 3)
    times = {k: [] for k in cases}
    for _ in range(repeats):
        for k, fn in cases.items():
            times[k].append(sample(fn, calls))
    return times


def report(times, unit):
    out = {k: stat(v, unit) for k, v in times.items()}
    for k in times:
        m = out[k]
        print(f"{k:40s} {m[f'median_{unit}']:10.2f} {unit} [{m[f'min_{unit}']:.2f}, {m[f'max_{unit}']:.2f}]", flush=True)
    return out


def decoder_part(a, dec):
    from sdfest_amd import _lib
    from sdfest_amd.differentiable_renderer import _stream
    L, h, dev = dec._L, dec._h, dec.device
    T = dec.latent_size
    z8 = torch.tensor(np.random.default_rng(0).normal(size=(8, T)).astype(np.float32), device=dev)
    z1 = z8[:1].contiguous()
    tape = torch.empty(L.sdfr_decoder_tape_bytes(h, 1) // 4, dtype=torch.float32, device=dev)
    dec._forward_raw(z1, False, tape)
    jac = torch.empty((1, 64 ** 3, (T + 3) & ~3), dtype=torch.float32, device=dev)
    ws = torch.empty(L.sdfr_decoder_jvp_workspace_bytes(h, 1, T), dtype=torch.uint8, device=dev)

    def jvp_call():
        _lib.check(L.sdfr_decoder_jvp(h, z1.data_ptr(), tape.data_ptr(), None, None, 1, T, 0, jac.data_ptr(), ws.data_ptr(),
                                      ws.numel(), _stream(dev)), "sdfr_decoder_jvp")
    with torch.no_grad():
        cases = {"decoder_jvp_n1_t8": jvp_call, "decoder_forward_8_latents": lambda: dec.decode(z8),
                 "SDFDecoder.jvp_n1_t8": lambda: dec.jvp(z1)}
        times = interleaved(cases, event_sample, a.calls, a.repeats)
    out = report(times, "us")
    out["jvp_over_forward_8"] = float(np.median(times["decoder_jvp_n1_t8"]) / np.median(times["decoder_forward_8_latents"]))
    print(f"jvp / forward of 8 latents = {out['jvp_over_forward_8']:.2f}", flush=True)
    return out


def kernel_part(a):
    from sdfest_amd import Camera, render_information
    from sdfest_amd.differentiable_renderer import forward_raw
    from sdfest_amd.synthetic import blobs_sdf, random_poses
    W, H, B, thr, T = 640, 480, a.views, 0.005, 8
    dev = torch.device("cuda:0")
    t = lambda x: torch.tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)
    sdf = t(blobs_sdf(0))
    pos, quat, isc = (t(x) for x in random_poses(B, seed=1, width=W, height=H, f=W / 2.0))
    cam = Camera(W, H, W / 2.0, W / 2.0, W / 2.0, H / 2.0, pixel_center=0.5)
    args = (W, H, W / 2.0, H / 2.0, W / 2.0, W / 2.0)
    depth = forward_raw(sdf, pos, quat, isc, *args, thr)
    target = forward_raw(sdf, pos + t([0.01, -0.008, 0.012]), quat, isc * 1.03, *args, thr)
    jac = t(np.random.default_rng(1).normal(size=(64 ** 3, T)))
    cases = {"render_information": lambda: render_information(depth, target, sdf, pos, quat, isc, cam),
             "render_information_shape_t8": lambda: render_information(depth, target, sdf, pos, quat, isc, cam,
                                                                       jacobian=jac, tangents=T)}
    g10, g = cases["render_information"](), cases["render_information_shape_t8"]()
    pick = list(range(8)) + [8 + T, 9 + T]
    agree = (g[:, pick][:, :, pick] - g10).abs().max().item() / g10.abs().max().item()   # faster and different is not faster
    times = interleaved(cases, event_sample, a.calls, a.repeats)
    out = report(times, "us")
    out["shape_over_pose"] = float(np.median(times["render_information_shape_t8"]) / np.median(times["render_information"]))
    out["included_pixels"] = int(g10[:, 9, 9].sum().item())
    out["max_abs_pose_block_minus_pose_call_over_max"] = agree
    print(f"shape / pose = {out['shape_over_pose']:.2f}; pose block vs the pose call: {agree:.2e} of its maximum", flush=True)
    return out


def pipeline_part(a, pipe):
    from _loop_scene import c5_scene
    image = c5_scene(views=1, max_iterations=a.iterations)["targets"][0]
    mask = image > 0
    depth = torch.where(mask, image, torch.full_like(image, 1.2)).contiguous()
    color = torch.zeros((480, 640, 3), device=depth.device)
    arg = torch.empty_like(depth)
    arg.copy_(depth)
    pipe(arg, mask, color)
    cases = {"pose_uncertainty": pipe.pose_uncertainty, "shape_uncertainty": pipe.shape_uncertainty,
             "shape_uncertainty_sdf_std": lambda: pipe.shape_uncertainty(sdf_std=True)}
    times = interleaved(cases, host_sample, max(1, a.calls // 4), a.repeats)
    out = report(times, "ms")
    out["shape_over_pose"] = float(np.median(times["shape_uncertainty"]) / np.median(times["pose_uncertainty"]))
    rec = pipe.shape_uncertainty()
    out["rank"] = int(rec.rank[0])
    out["position_std_m"] = {"marginal": rec.position_std[0].tolist(), "conditional": rec.conditional.position_std[0].tolist()}
    out["scale_rel_std"] = {"marginal": float(rec.scale_rel_std[0]), "conditional": float(rec.conditional.scale_rel_std[0])}
    print(f"shape / pose uncertainty = {out['shape_over_pose']:.2f}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--calls", type=int, default=20, help="calls per sample")
    ap.add_argument("--repeats", type=int, default=15, help="interleaved rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_shape_information.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shape_information.py measures on the GPU; none found")
    from bench_hypotheses import pipeline
    pipe = pipeline(a.iterations)
    results = {"decoder": decoder_part(a, pipe.vae), "kernel": kernel_part(a), "pipeline": pipeline_part(a, pipe)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "image": [640, 480], "views": a.views, "tangents": 8,
                   "iterations": a.iterations, "calls_per_sample": a.calls, "repeats": a.repeats, "interleaved": True,
                   "what": "decoder, kernel: device events around calls_per_sample calls, us per call (every launch of "
                           "the call, plus the wrappers' allocations where the case is a Python wrapper); pipeline: host "
                           "clock around calls that end in a device synchronise; the first two samples of every case are "
                           "not timed",
                   "results": results}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
