#!/usr/bin/env python3
"""What the oriented boxes cost: ``sdfr_box_iou`` and ``sdfr_sdf_bounds`` (csrc/boxes.hip) on the device.

Part 1: ``box_iou`` for 5 pairs, a 64 x 64 and a 1024 x 1024 matrix of seeded random boxes (side lengths in [0.05, 0.5],
centres N(0, 0.15^2) about each other -- three quarters of such pairs overlap), without and with 20 symmetry steps, beside
the numpy twin (tests/box_iou_twin.py) on the 5 pairs (host clock).  The inputs are float64 columns already on the device;
a call is the Python wrapper (six conversions, two concatenations, two allocations) and the launch, so the small cases
measure the wrapper.
Part 2: ``sdf_bounds`` for 1, 32 and 256 grids of 64^3 (the mug decoder's volumes at seeded latents, level 0.02, padded)
beside ``sdfr_mesh_count`` + ``sdfr_mesh_emit`` on the same grids (``extract_mesh`` with its host read of the counts:
host clock around a synchronise) and beside a device copy of the same bytes (``Tensor.copy_``, read + write).
Part 3 (accuracy, no timing): a 0.1 x 0.07 x 0.16 box against itself turned by d about a generic axis, for d from 1e-3
to 1e-13 rad -- faces that cross at the angle d.  The same second box given turned half about its own y axis is the same
set of points, so the two volumes differ by what the clipping loses: their difference over the volume, and 1 - V / V_a.
A device sample is `--calls` consecutive calls between two device events; everything is warmed up and the samples are
INTERLEAVED (`--repeats` rounds).  Medians and ranges go to profiles/bench_boxes.json."""
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


def stat(ts, unit="us"):
    k = {"us": 1e6, "ms": 1e3}[unit]
    return {f"median_{unit}": float(np.median(ts)) * k, f"min_{unit}": float(min(ts)) * k, f"max_{unit}": float(max(ts)) * k}


def interleaved(samplers, repeats):
    """{name: [seconds]}: one sample of every entry per round"""
    for fn in samplers.values():
        fn()
    out = {name: [] for name in samplers}
    for _ in range(repeats):
        for name, fn in samplers.items():
            out[name].append(fn())
    return out


def random_boxes(n, rng, about=None):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    c = rng.normal(size=(n, 3)) if about is None else about + rng.normal(size=(n, 3)) * 0.15
    return np.concatenate([c, q, rng.uniform(0.05, 0.5, (n, 3))], 1)


def iou_part(a):
    import box_iou_twin as twin
    from sdfest_amd import box_iou
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    results = {}
    for label, n, paired in (("5 pairs", 5, True), ("64 x 64", 64, False), ("1024 x 1024", 1024, False)):
        A = random_boxes(n, rng, about=np.zeros(3))
        B = random_boxes(n, rng, about=A[:, :3] if paired else np.zeros(3))
        ta, tb = (torch.tensor(x, device=dev) for x in (A, B))
        call = lambda **kw: box_iou(ta[:, :3], ta[:, 3:7], ta[:, 7:], tb[:, :3], tb[:, 3:7], tb[:, 7:], paired=paired, **kw)
        calls = max(1, a.calls // (16 if n == 1024 else 1))
        samplers = {"plain": lambda: event_sample(call, calls),
                    "20 steps about z": lambda: event_sample(lambda: call(rotational_symmetry_axis=2), calls)}
        ts = interleaved(samplers, a.repeats)
        iou = call().cpu().numpy()
        entry = {"pairs": int(iou.size), "overlapping_share": float((iou > 0).mean()),
                 "plain": stat(ts["plain"]), "symmetry_20": stat(ts["20 steps about z"])}
        if paired:
            boxes = lambda X: [(r[:3], r[3:7], r[7:]) for r in X]
            twin_ts = {"plain": [], "symmetry_20": []}
            for _ in range(3):
                for name, kw in (("plain", {}), ("symmetry_20", {"symmetry_axis": 2, "symmetry_steps": 20})):
                    t0 = time.perf_counter()
                    ref = [twin.box_intersection(x, y, **kw)[1] for x, y in zip(boxes(A), boxes(B))]
                    twin_ts[name].append(time.perf_counter() - t0)
            entry["numpy_twin"] = {name: stat(v, "ms") for name, v in twin_ts.items()}
        results[label] = entry
        print(label, json.dumps(entry))
    return results


def bounds_part(a):
    import _loop_scenes as S
    from sdfest_amd import extract_mesh, sdf_bounds
    dev = torch.device("cuda:0")
    dec, d = S.mug_decoder()
    rng = np.random.default_rng(12)
    level = 0.02
    results = {}
    for n in (1, 32, 256):
        z = torch.tensor(d["z"][rng.integers(0, len(d["z"]), n)] * rng.uniform(0.3, 0.8, (n, 1)), dtype=torch.float32,
                         device=dev)
        with torch.no_grad():
            sdf = torch.cat([dec.decode(z[i:i + 32])[:, 0] for i in range(0, n, 32)]).contiguous()
        other = torch.empty_like(sdf)
        calls = max(1, a.calls // (8 if n == 256 else 1))
        samplers = {"bounds": lambda: event_sample(lambda: sdf_bounds(sdf, level, complete=True), calls),
                    "copy": lambda: event_sample(lambda: other.copy_(sdf), calls),
                    "mesh": lambda: host_sample(lambda: extract_mesh(sdf, level, complete=True), max(1, calls // 8))}
        ts = interleaved(samplers, a.repeats)
        lo, hi, crossed = sdf_bounds(sdf, level, complete=True)
        nbytes = sdf.numel() * 4
        b, c = float(np.median(ts["bounds"])), float(np.median(ts["copy"]))
        entry = {"grids": n, "bytes_read": nbytes, "crossed_edges_mean": float(crossed.float().mean()),
                 "bounds": stat(ts["bounds"]), "copy": stat(ts["copy"]), "mesh_count_emit": stat(ts["mesh"]),
                 "bounds_read_GBps": nbytes / b * 1e-9, "copy_read_GBps": nbytes / c * 1e-9,
                 "share_of_copy_rate": c / b}
        results[f"{n} x 64^3"] = entry
        print(n, json.dumps(entry))
    return results


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def near_parallel_part():
    from sdfest_amd import box_iou
    q = np.array([0.3, -0.2, 0.1, 0.9])
    q /= np.linalg.norm(q)
    p, e = np.array([0.0, 0.0, -0.6]), np.array([0.1, 0.07, 0.16])
    axis = np.array([0.5, -0.3, 0.8])
    axis /= np.linalg.norm(axis)
    results = {}
    for d in (1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9, 1e-10, 1e-11, 1e-12, 1e-13):
        turned = qmul(q, np.append(np.sin(d / 2) * axis, np.cos(d / 2)))
        half = qmul(turned, [0.0, 1.0, 0.0, 0.0])
        _, v = box_iou(p, q, e, np.stack([p, p]), np.stack([turned, half]), np.stack([e, e]), return_intersection=True)
        v = v.cpu().numpy()[0]
        results[f"{d:g}"] = {"loss": float(1 - v[0] / e.prod()), "half_turn_difference": float(abs(v[0] - v[1]) / e.prod())}
        print(f"{d:g}", json.dumps(results[f"{d:g}"]))
    return results


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=64, help="calls per device sample")
    ap.add_argument("--repeats", type=int, default=15, help="interleaved rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_boxes.json"))
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "repeats": a.repeats,
              "box_iou": iou_part(a), "sdf_bounds": bounds_part(a),
              "near_parallel_faces": near_parallel_part()}
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("written", a.out)


if __name__ == "__main__":
    main()
