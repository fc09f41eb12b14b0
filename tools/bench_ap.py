#!/usr/bin/env python3
"""What average precision costs: ``sdfr_pose_pair_errors``, ``sdfr_ap_match`` and ``sdfr_ap_integrate`` (csrc/ap.hip) and
the whole ``mean_average_precision`` call on a REAL275-sized synthetic result set.

The set: 2 754 frames of 6 ground truths each, classes drawn from 6 (so a (frame, class) group holds one to a few
objects), one class symmetric about its y axis; a detection per ground truth moved by N(0, 2 cm), turned by up to 30
degrees and rescaled by up to 15 %, a tenth of them missing and as many spurious ones added; distinct scores.  101 IoU
criteria (0, 0.01 .. 1) and 61 x 31 pose criteria (0 .. 60 degrees, 0 .. 15 cm).
Device samples are `--calls` consecutive calls between two device events, the whole call is on the host clock around a
synchronise (it reads sizes and the result back); everything is warmed up and the samples are INTERLEAVED (`--repeats`
rounds); medians and ranges.  Beside them the numpy twin (tests/ap_twin.py) on the first `--twin-frames` frames of the same
set, with the SAME criteria, given the device's IoU values per pair (so its time leaves the box intersections out), on
the host clock, once.  Everything goes to profiles/bench_ap.json."""
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

FRAMES, PER_FRAME, CLASSES, SYMMETRIC_CLASS = 2754, 6, 6, 3
IOU_T = [round(0.01 * k, 2) for k in range(101)]
DEG_T = [float(k) for k in range(61)]
DIST_T = [round(0.005 * k, 3) for k in range(31)]


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


def qmul(a, b):
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], 1)


def result_set(frames, seed=31):
    rng = np.random.default_rng(seed)
    n = frames * PER_FRAME
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    gt = {"frame": np.repeat(np.arange(frames), PER_FRAME), "class_id": rng.integers(1, CLASSES + 1, n),
          "position": np.concatenate([rng.uniform(-0.4, 0.4, (n, 2)), rng.uniform(-1.5, -0.6, (n, 1))], 1),
          "orientation": unit(rng.normal(size=(n, 4))), "extents": rng.uniform(0.08, 0.3, (n, 3))}
    gt["symmetry_axis"] = np.where(gt["class_id"] == SYMMETRIC_CLASS, 1, -1)
    keep = rng.random(n) >= 0.1
    half = np.deg2rad(rng.uniform(0.0, 30.0, n)) / 2
    turn = np.concatenate([unit(rng.normal(size=(n, 3))) * np.sin(half)[:, None], np.cos(half)[:, None]], 1)
    det = {"frame": gt["frame"][keep], "class_id": gt["class_id"][keep],
           "position": (gt["position"] + rng.normal(size=(n, 3)) * 0.02)[keep],
           "orientation": qmul(gt["orientation"], turn)[keep], "extents": (gt["extents"] * rng.uniform(0.85, 1.15, (n, 3)))[keep]}
    m = n - int(keep.sum())
    extra = {"frame": rng.integers(0, frames, m), "class_id": rng.integers(1, CLASSES + 1, m),
             "position": np.concatenate([rng.uniform(-0.4, 0.4, (m, 2)), rng.uniform(-1.5, -0.6, (m, 1))], 1),
             "orientation": unit(rng.normal(size=(m, 4))), "extents": rng.uniform(0.08, 0.3, (m, 3))}
    det = {k: np.concatenate([det[k], extra[k]]) for k in det}
    det["score"] = rng.permutation(len(det["frame"])) / len(det["frame"])
    return det, gt


def main():
    ap_ = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap_.add_argument("--frames", type=int, default=FRAMES)
    ap_.add_argument("--calls", type=int, default=8, help="calls per device sample")
    ap_.add_argument("--repeats", type=int, default=11, help="interleaved rounds")
    ap_.add_argument("--twin-frames", type=int, default=28, help="frames the numpy twin scores (about 1 %% of the set)")
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_ap.json"))
    a = ap_.parse_args()
    import ap_twin as twin
    from sdfest_amd import ap, mean_average_precision
    dev = torch.device("cuda:0")
    det, gt = result_set(a.frames)
    to_dev = lambda d: {k: torch.tensor(v, device=dev) for k, v in d.items()}
    det_d, gt_d = to_dev(det), to_dev(gt)
    groups = ap.group_detections(det_d["frame"], det_d["class_id"], det_d["score"], gt_d["frame"], gt_d["class_id"], dev)
    table, _ = ap.pair_table(det_d, gt_d, groups)
    pose_table = ap.with_key(table, "pose")
    inf = float("inf")
    iou_criteria = torch.tensor([(t, inf, inf) for t in IOU_T], dtype=torch.float64, device=dev)
    pose_criteria = torch.tensor([(-inf, d, s) for d in DEG_T for s in DIST_T], dtype=torch.float64, device=dev)
    iou_matched = ap.match_detections(table, groups, iou_criteria)
    pose_matched = ap.match_detections(pose_table, groups, pose_criteria)
    pg, pd = groups.pair_gt, groups.pair_det
    f64 = lambda d, k: d[k].to(torch.float64)
    pose_a = torch.cat([f64(gt_d, "position")[pg], f64(gt_d, "orientation")[pg]], 1)
    pose_b = torch.cat([f64(det_d, "position")[pd], f64(det_d, "orientation")[pd]], 1)
    axis = gt_d["symmetry_axis"][pg].to(torch.int32)
    L = ap._lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def raw_match(tab, crit, out):   # the entry point alone: no allocation, no status read
        return lambda: L.sdfr_ap_match(tab.data_ptr(), groups.n_pairs, groups.pred_offset.data_ptr(),
                                       groups.gt_offset.data_ptr(), groups.pair_offset.data_ptr(), groups.G, groups.P,
                                       crit.data_ptr(), int(crit.shape[0]), out.data_ptr(), status.data_ptr(), 0, stream)

    samplers = {
        "pose_pair_errors": lambda: event_sample(lambda: ap.pose_pair_errors(pose_a, pose_b, axis), a.calls),
        "pair_table": lambda: event_sample(lambda: ap.pair_table(det_d, gt_d, groups), a.calls),
        "match_iou": lambda: event_sample(raw_match(table, iou_criteria, iou_matched), a.calls),
        "match_pose": lambda: event_sample(raw_match(pose_table, pose_criteria, pose_matched), a.calls),
        "integrate_iou": lambda: event_sample(lambda: ap.average_precision(iou_matched, groups), a.calls),
        "integrate_pose": lambda: event_sample(lambda: ap.average_precision(pose_matched, groups), a.calls),
        "copy_of_pose_matched": lambda: event_sample(lambda: pose_matched.clone(), a.calls),
        "group_detections": lambda: host_sample(lambda: ap.group_detections(
            det_d["frame"], det_d["class_id"], det_d["score"], gt_d["frame"], gt_d["class_id"], dev), 1),
        "mean_average_precision": lambda: host_sample(
            lambda: mean_average_precision(det_d, gt_d, IOU_T, DEG_T, DIST_T), 1),
        "mean_average_precision_from_numpy": lambda: host_sample(
            lambda: mean_average_precision(det, gt, IOU_T, DEG_T, DIST_T), 1),
    }
    ts = interleaved(samplers, a.repeats)
    sizes = torch.diff(groups.pred_offset).cpu().numpy(), torch.diff(groups.gt_offset).cpu().numpy()
    Tp, Ti, P = int(pose_criteria.shape[0]), int(iou_criteria.shape[0]), groups.P
    med = lambda name: float(np.median(ts[name]))
    result = {
        "device": torch.cuda.get_device_name(0), "calls": a.calls, "repeats": a.repeats,
        "set": {"frames": a.frames, "detections": P, "ground_truths": int(len(gt["frame"])), "classes": groups.C,
                "groups": groups.G, "pairs": groups.n_pairs, "largest_group": [int(sizes[0].max()), int(sizes[1].max())],
                "iou_criteria": Ti, "pose_criteria": Tp, "matched_share_pose": float((pose_matched != 255).float().mean())},
        "device_us": {k: stat(ts[k]) for k in ("pose_pair_errors", "pair_table", "match_iou", "match_pose",
                                               "integrate_iou", "integrate_pose", "copy_of_pose_matched")},
        "host_ms": {k: stat(ts[k], "ms") for k in ("group_detections", "mean_average_precision",
                                                   "mean_average_precision_from_numpy")},
        # the traffic the layout asks for: matched [T][P] written once by the matching, read twice by the integral
        "match_pose_threads": Tp * groups.G,
        "match_pose_ns_per_thread": med("match_pose") / (Tp * groups.G) * 1e9,
        "match_pose_written_GBps": Tp * P / med("match_pose") * 1e-9,
        "integrate_pose_read_GBps": 2 * Tp * P / med("integrate_pose") * 1e-9,
        "copy_read_plus_write_GBps": 2 * Tp * P / med("copy_of_pose_matched") * 1e-9,
    }
    # the twin on the first frames, the same criteria, the device's IoU per pair
    keep_d, keep_g = det["frame"] < a.twin_frames, gt["frame"] < a.twin_frames
    det_s, gt_s = {k: v[keep_d] for k, v in det.items()}, {k: v[keep_g] for k, v in gt.items()}
    iou_of = {}
    h = torch.stack([pd.double(), pg.double(), table[:, 0]], 1).cpu().numpy()
    index_d, index_g = np.cumsum(keep_d) - 1, np.cumsum(keep_g) - 1
    for i, j, v in h:
        if keep_d[int(i)] and keep_g[int(j)]:
            iou_of[(int(index_d[int(i)]), int(index_g[int(j)]))] = v
    t0 = time.perf_counter()
    ref = twin.mean_average_precision(det_s, gt_s, IOU_T, DEG_T, DIST_T, pair_iou=lambda i, j: iou_of[(i, j)])
    twin_s = time.perf_counter() - t0
    got = mean_average_precision(det_s, gt_s, IOU_T, DEG_T, DIST_T)
    result["numpy_twin"] = {"frames": a.twin_frames, "share_of_the_set": a.twin_frames / a.frames, "seconds": twin_s,
                            "scaled_to_the_set_seconds": twin_s * a.frames / a.twin_frames,
                            "without": "the box intersections (the device's IoU values are handed to it)",
                            "worst_ap_difference": float(max(np.nanmax(np.abs(got["iou_ap"] - ref["iou_ap"])),
                                                             np.nanmax(np.abs(got["pose_ap"] - ref["pose_ap"]))))}
    full = mean_average_precision(det_d, gt_d, IOU_T, DEG_T, DIST_T)
    pick = lambda ts_, v: ts_.index(v)
    result["values"] = {"iou_map_25_50_75": [float(full["iou_map"][pick(IOU_T, v)]) for v in (0.25, 0.5, 0.75)],
                        "pose_map_5deg_5cm": float(full["pose_map"][pick(DEG_T, 5.0), pick(DIST_T, 0.05)]),
                        "pose_map_10deg_5cm": float(full["pose_map"][pick(DEG_T, 10.0), pick(DIST_T, 0.05)])}
    print(json.dumps(result, indent=1))
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("written", a.out)


if __name__ == "__main__":
    main()
