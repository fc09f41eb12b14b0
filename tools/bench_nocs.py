#!/usr/bin/env python3
"""Time the NOCS annotation of the fixture frame (tests/golden/nocs_frame.npz: five objects of 3 168 - 5 078
correspondences): the similarity fits (sample indices + ``sdfr_similarity_ransac``) of its five objects as ONE call,
as FIVE calls, and replicated to 64 frames (320 objects) per call; the frame's correspondences
(``sdfr_nocs_count`` + ``sdfr_nocs_correspondences``, including their one read-back); and the numpy twin's
(tests/nocs_twin.py) five fits on this machine's CPU, host clock.

Device events around `--iters` calls after `--warmup`, `--repeats` times, the forms alternating; medians and ranges go
to profiles/bench_nocs.json.  There is no target ratio; the run FAILS unless the one-call form is faster than the twin's
five fits measured in the same run.  Reads nothing outside the repository.
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_nocs.json"))
    a = ap.parse_args()
    import nocs_twin as tw
    from sdfest_amd import Camera
    from sdfest_amd import nocs_utils as nu
    if not torch.cuda.is_available():
        raise SystemExit("bench_nocs.py needs a GPU")
    dev = torch.device("cuda", 0)
    f = np.load(os.path.join(ROOT, "tests", "golden", "nocs_frame.npz"))
    depth = f["depth_mm"].astype(np.float32) * np.float32(0.001)
    ids = [int(i) for i in f["meta_mask_id"]]
    cam = Camera(**tw.REAL_CAMERA)
    d_depth, d_mask, d_coord = (torch.tensor(x, device=dev) for x in (depth, f["mask"], f["coord"]))
    c = nu.nocs_correspondences(d_depth, d_mask, d_coord, ids, cam)
    offsets = np.concatenate([[0], np.cumsum(c.counts)]).tolist()
    seeds = torch.tensor([tw.object_seed(0, 0, i) for i in ids], dtype=torch.int64, device=dev)
    parts = [(c.source[a0:b0].contiguous(), c.target[a0:b0].contiguous(), seeds[k:k + 1])
             for k, (a0, b0) in enumerate(zip(offsets[:-1], offsets[1:]))]
    F = a.frames
    many_s, many_t = c.source.repeat(F, 1), c.target.repeat(F, 1)
    many_off = np.concatenate([[0], np.cumsum(c.counts * F)]).tolist()
    many_seeds = seeds.repeat(F)

    def one_call():
        return nu.estimate_similarity_transforms(c.source, c.target, offsets, object_seeds=seeds)

    def five_calls():
        return [nu.estimate_similarity_transforms(s, t, [0, len(s)], object_seeds=k) for s, t, k in parts]

    def many_frames():
        return nu.estimate_similarity_transforms(many_s, many_t, many_off, object_seeds=many_seeds)

    def correspondences():
        return nu.nocs_correspondences(d_depth, d_mask, d_coord, ids, cam)

    # the same objects, the same draws, in numpy: results first (they must agree), then the time
    r = one_call()
    host = [(tw.correspondences(depth, f["mask"], f["coord"], i)[:2], tw.sample_indices(n, tw.object_seed(0, 0, i)))
            for i, n in zip(ids, c.counts)]
    status, T = r.status.cpu().tolist(), r.transform.cpu().numpy()
    for k, ((s, t), draws) in enumerate(host):
        o = tw.ransac(s, t, draws)
        assert status[k] == o["status"] == tw.OK and np.max(np.abs(T[k] - o["transform"])) < 1e-9, k
    m = many_frames()
    assert torch.equal(m.transform.view(F, 5, 4, 4)[F - 1], r.transform), "a replicated frame differs from the frame"
    twin_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        for (s, t), draws in host:
            tw.ransac(s, t, draws)
        twin_ms.append((time.perf_counter() - t0) * 1e3)

    forms = {"one_call": one_call, "five_calls": five_calls, f"frames_{F}": many_frames,
             "correspondences": correspondences}
    for fn in forms.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, fn in forms.items():
            times[k].append(timed(fn, a.iters if k != f"frames_{F}" else max(a.iters // 5, 2)))
    med = {k: float(np.median(v)) for k, v in times.items()}
    result = {
        "device": torch.cuda.get_device_name(0), "objects": 5, "correspondences_per_object": c.counts,
        "iters": a.iters, "repeats": a.repeats,
        "ms": {k: {"median": med[k], "min": float(min(v)), "max": float(max(v))} for k, v in times.items()},
        "ms_per_frame_at_%d_frames" % F: med[f"frames_{F}"] / F,
        "twin_numpy_five_fits_ms": {"median": float(np.median(twin_ms)), "min": min(twin_ms), "max": max(twin_ms)},
        "twin_over_one_call": float(np.median(twin_ms)) / med["one_call"],
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))
    if not med["one_call"] < float(np.median(twin_ms)):
        raise SystemExit("the one-call form is not faster than the numpy twin's five fits")


if __name__ == "__main__":
    main()
