#!/usr/bin/env python3
"""Time the annotated-frame path at 640 x 480 on a generated set (tests/redwood_scenes.py with the Redwood camera: 16
frames of the mug sequence): ``AnnotatedRedwoodDataset.samples`` of 1 and of 16 frames (host clock, the PNG decoding
included, the device drained) with the mask pass alone beside it (``visible_mask`` of 1 and 16 images as Python calls
it, and ``sdfr_visible_mask`` on buffers made beforehand for 1, 16 and 64 images: device events around `--iters` calls),
and ``evaluate_annotated`` with the mug pipeline in samples per second at ``frames_per_call`` 1 and 8.

Medians and ranges go to profiles/bench_redwood.json.  The tool records numbers and sets no threshold.  Reads nothing
outside the repository; the set is written to a temporary folder.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

CAMERA = {"width": 640, "height": 480, "fx": 525.0, "fy": 525.0, "cx": 319.5, "cy": 239.5, "pixel_center": 0.0}
FRAMES = 16


def device_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-iterations", type=int, default=30)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_redwood.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_redwood.py needs a GPU")
    import redwood_scenes
    from rendering_evaluation import DEFAULTS, build_pipeline
    from sdfest_amd import AnnotatedRedwoodDataset, _lib, visible_mask
    from sdfest_amd.evaluation import evaluate_annotated
    rng = np.random.default_rng(0)
    poses = []
    for n in range(FRAMES):
        q = rng.normal(size=4)
        poses.append(([float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.06, 0.06)), float(rng.uniform(0.45, 0.6))],
                      (q / np.linalg.norm(q)).tolist()))
    result = {"device": torch.cuda.get_device_name(0), "camera": CAMERA, "frames": FRAMES, "iters": a.iters,
              "repeats": a.repeats}
    with tempfile.TemporaryDirectory() as folder:
        scene = redwood_scenes.write_scene(folder, CAMERA, {"seq_mug": poses})
        ds = AnnotatedRedwoodDataset({"root_dir": scene["root_dir"], "ann_dir": scene["ann_dir"], "camera": CAMERA,
                                      "camera_convention": "opencv", "mask_pointcloud": True})
        # ---- samples() and the mask kernel ---------------------------------------------------------------------------
        ds.samples(range(FRAMES))       # the mesh is read, the kernels are loaded
        one = [host_ms(lambda: ds.samples([n % FRAMES])) for n in range(a.repeats * 4)]
        many = [host_ms(lambda: ds.samples(range(FRAMES))) for _ in range(a.repeats)]
        frames = ds.samples(range(FRAMES))
        observed = torch.stack([f["depth"] for f in frames])
        rendered = torch.where(torch.stack([f["mask"] for f in frames]), observed, torch.zeros_like(observed))
        kernel = {}
        for B in (1, FRAMES):
            r, o = rendered[:B].contiguous(), observed[:B].contiguous()
            fn = lambda: visible_mask(r, o, 0.01, return_masked=True, return_counts=True)
            fn()
            kernel[B] = [device_ms(fn, a.iters) for _ in range(a.repeats)]
        # the entry point alone on buffers made beforehand (the count fill and the kernel: two launches), 64 images too
        raw = {}
        for B in (1, FRAMES, 4 * FRAMES):
            r = rendered.repeat(-(-B // FRAMES), 1, 1)[:B].contiguous()
            o = observed.repeat(-(-B // FRAMES), 1, 1)[:B].contiguous()
            mask, masked = torch.empty_like(r, dtype=torch.bool), torch.empty_like(r)
            counts = torch.empty((B, 4), dtype=torch.int32, device=r.device)
            st = torch.cuda.current_stream().cuda_stream
            fn = lambda: _lib.check(_lib.lib().sdfr_visible_mask(r.data_ptr(), o.data_ptr(), B, 480, 640, 0.01,
                                                                 mask.data_ptr(), masked.data_ptr(), counts.data_ptr(),
                                                                 r.device.index, st), "sdfr_visible_mask")
            fn()
            raw[B] = [device_ms(fn, a.iters) for _ in range(a.repeats)]
        result["samples_ms"] = {"1": spread(one), str(FRAMES): spread(many)}
        result["visible_mask_call_ms"] = {str(B): spread(v) for B, v in kernel.items()}
        result["sdfr_visible_mask_ms"] = {str(B): spread(v) for B, v in raw.items()}
        bytes_per_pixel = 13       # 8 read, 1 + 4 written (mask and masked)
        result["sdfr_visible_mask_GBps"] = {str(B): bytes_per_pixel * B * 640 * 480 / (np.median(v) * 1e-3) / 1e9
                                            for B, v in raw.items()}
        # ---- evaluate_annotated --------------------------------------------------------------------------------------
        cfg = dict(DEFAULTS, camera=CAMERA, max_iterations=a.max_iterations, threshold=0.005, iso_threshold=0.0)
        pipe = build_pipeline(cfg, os.path.join(ROOT, "tests", "golden", "mug_decoder_weights.npz"), None)
        rates = {}
        for K in (1, 8):
            run = lambda: evaluate_annotated(pipe, ds, a.points, 0, frames_per_call=K)
            out = run()                  # builds and captures the loop of K rows
            assert len(out["samples"]) == FRAMES and not out["skipped"]
            rates[K] = [FRAMES / (host_ms(run) * 1e-3) for _ in range(a.repeats)]
        result["evaluate_annotated_samples_per_s"] = {str(K): spread(v) for K, v in rates.items()}
        result["evaluate_annotated_8_over_1"] = float(np.median(rates[8]) / np.median(rates[1]))
        result["max_iterations"], result["points"] = a.max_iterations, a.points
        # the estimation alone, per frame: what frames_per_call can speed up (the rest -- loading, meshes, samples,
        # metrics -- is done frame by frame either way)
        depth = torch.stack([f["depth"] for f in frames[:8]])
        masks = torch.stack([f["mask"] for f in frames[:8]])
        color = frames[0]["color"]
        single = lambda: [pipe(depth[k].clone(), masks[k], color) for k in range(8)]
        together = lambda: pipe.estimate_frames(depth.clone(), masks)
        single(), together()
        result["estimate_ms_per_frame"] = {"call": spread([host_ms(single) / 8 for _ in range(a.repeats)]),
                                           "estimate_frames_8": spread([host_ms(together) / 8 for _ in range(a.repeats)])}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
