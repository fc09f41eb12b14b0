#!/usr/bin/env python3
"""Average precision of a folder of per-frame detection results (``sdfest_amd.mean_average_precision``, DESIGN.md
section 3.22): AP per class over IoU thresholds and over (degrees, distance) thresholds, their means over the classes, a
table on the terminal and everything as JSON.

Every ``*.pkl`` of the folder is one frame (sorted by name) and holds a dict with the keys
    gt_class_ids (G,), gt_RTs (G,4,4), gt_scales (G,3), gt_handle_visibility (G,)   [the last one is optional]
    pred_class_ids (P,), pred_scores (P,), pred_RTs (P,4,4), pred_scales (P,3)
An ``RT`` is a 4 x 4 similarity transform object -> camera: s = cbrt(det(RT[:3,:3])) is its scale, RT[:3,:3] / s the
rotation, RT[:3,3] the position in metres, and the box's full side lengths are ``scales * s``.
THIS LAYOUT IS RESTATED FROM MEMORY of the result files the NOCS evaluation reads; it is not pinned against such files or
against that evaluation's script, and the protocol is this project's own (include/sdfr.h group 16): no parity is claimed.

--symmetric-classes: class ids whose turn about --symmetry-axis (of the object's own frame; 1 = y) cannot be observed;
--handle-class: a class that is symmetric only in the frames where ``gt_handle_visibility`` is 0 (a mug whose handle is
hidden)."""
import argparse
import glob
import json
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def decompose(rts):
    """(positions (N,3), quaternions (N,4) x y z w, scales (N,)) of N similarity transforms (N,4,4)"""
    from sdfest_amd.nocs_dataset import matrix_to_quaternion
    rts = np.asarray(rts, np.float64).reshape(-1, 4, 4)
    scale = np.cbrt(np.linalg.det(rts[:, :3, :3])) if len(rts) else np.zeros(0)
    quat = np.array([matrix_to_quaternion(rt[:3, :3] / s) for rt, s in zip(rts, scale)]).reshape(-1, 4)
    return rts[:, :3, 3].copy(), quat, scale


def load_results(folder, symmetric_classes=(), symmetry_axis=1, handle_class=None):
    """(detections, ground_truths, number of frames): the dicts of ``mean_average_precision`` from the pickles of
    `folder`; the frame id is the file's place in the sorted listing"""
    files = sorted(glob.glob(os.path.join(folder, "*.pkl")))
    if not files:
        raise FileNotFoundError(f"no *.pkl in {folder}")
    det = {k: [] for k in ("frame", "class_id", "score", "position", "orientation", "extents")}
    gt = {k: [] for k in ("frame", "class_id", "position", "orientation", "extents", "symmetry_axis")}
    for frame, path in enumerate(files):
        with open(path, "rb") as fh:
            r = pickle.load(fh)
        for d, prefix in ((gt, "gt"), (det, "pred")):
            ids = np.asarray(r[f"{prefix}_class_ids"], np.int64).reshape(-1)
            position, quat, scale = decompose(r[f"{prefix}_RTs"])
            extents = np.asarray(r[f"{prefix}_scales"], np.float64).reshape(-1, 3) * scale[:, None]
            if not (len(ids) == len(position) == len(extents)):
                raise ValueError(f"{path}: {len(ids)} {prefix} class ids, {len(position)} transforms, {len(extents)} scales")
            d["frame"].append(np.full(len(ids), frame, np.int64)), d["class_id"].append(ids)
            d["position"].append(position), d["orientation"].append(quat), d["extents"].append(extents)
        ids = gt["class_id"][-1]
        symmetric = np.isin(ids, list(symmetric_classes))
        if handle_class is not None and "gt_handle_visibility" in r:
            hidden = np.asarray(r["gt_handle_visibility"]).reshape(-1) == 0
            symmetric |= (ids == handle_class) & hidden
        gt["symmetry_axis"].append(np.where(symmetric, symmetry_axis, -1).astype(np.int64))
        det["score"].append(np.asarray(r["pred_scores"], np.float64).reshape(-1))
    return {k: np.concatenate(v) for k, v in det.items()}, {k: np.concatenate(v) for k, v in gt.items()}, len(files)


def print_table(out, iou_t, deg_t, dist_t):
    names = [f"class {c}" for c in out["classes"]] + ["mAP"]
    rows = lambda per_class, mean: list(per_class) + [mean]
    print("IoU".ljust(12) + "".join(f"{t:>9.2f}" for t in iou_t))
    for name, row in zip(names, rows(out["iou_ap"], out["iou_map"])):
        print(name.ljust(12) + "".join(f"{100 * v:>9.1f}" for v in row))
    for i, d in enumerate(deg_t):
        print(f"{d:g} degrees".ljust(12) + "".join(f"{100 * s:>7.1f}cm" for s in dist_t))
        for name, row in zip(names, rows(out["pose_ap"][:, i], out["pose_map"][i])):
            print(name.ljust(12) + "".join(f"{100 * v:>9.1f}" for v in row))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("folder", help="the folder of per-frame *.pkl results")
    ap.add_argument("--out", default=None, help="the JSON file to write (default: FOLDER/average_precision.json)")
    ap.add_argument("--symmetric-classes", type=int, nargs="*", default=[], help="class ids that are rotationally symmetric")
    ap.add_argument("--symmetry-axis", type=int, default=1, choices=(0, 1, 2), help="their axis, in the object's frame")
    ap.add_argument("--handle-class", type=int, default=None,
                    help="a class that is symmetric where gt_handle_visibility is 0")
    ap.add_argument("--iou-thresholds", type=float, nargs="+", default=[round(0.01 * k, 2) for k in range(101)])
    ap.add_argument("--degree-thresholds", type=float, nargs="+", default=[float(k) for k in range(61)])
    ap.add_argument("--distance-thresholds", type=float, nargs="+", default=[round(0.005 * k, 3) for k in range(31)],
                    help="metres")
    ap.add_argument("--iou-min-for-pose", type=float, default=None,
                    help="the pose criteria also ask for this IoU (default: no overlap test)")
    ap.add_argument("--symmetry-steps", type=int, default=20, help="turns tried by the IoU of a symmetric object")
    a = ap.parse_args()
    from sdfest_amd import mean_average_precision
    det, gt, frames = load_results(a.folder, a.symmetric_classes, a.symmetry_axis, a.handle_class)
    out = mean_average_precision(det, gt, a.iou_thresholds, a.degree_thresholds, a.distance_thresholds,
                                 iou_min_for_pose=a.iou_min_for_pose, symmetry_steps=a.symmetry_steps)
    shown = lambda ts, picks: [t for t in ts if any(abs(t - p) < 1e-9 for p in picks)] or list(ts)[:6]
    iou_s, deg_s, dist_s = shown(a.iou_thresholds, (0.25, 0.5, 0.75)), shown(a.degree_thresholds, (5, 10)), \
        shown(a.distance_thresholds, (0.02, 0.05, 0.1))
    pick = lambda ts, sub: [list(ts).index(t) for t in sub]
    view = {"classes": out["classes"], "iou_ap": out["iou_ap"][:, pick(a.iou_thresholds, iou_s)],
            "iou_map": out["iou_map"][pick(a.iou_thresholds, iou_s)],
            "pose_ap": out["pose_ap"][:, pick(a.degree_thresholds, deg_s)][:, :, pick(a.distance_thresholds, dist_s)],
            "pose_map": out["pose_map"][pick(a.degree_thresholds, deg_s)][:, pick(a.distance_thresholds, dist_s)]}
    print(f"{frames} frames, {len(det['frame'])} detections, {len(gt['frame'])} ground truths; AP in percent")
    print_table(view, iou_s, deg_s, dist_s)
    result = {k: v.tolist() for k, v in out.items()}
    result.update(frames=frames, iou_thresholds=list(a.iou_thresholds), degree_thresholds=list(a.degree_thresholds),
                  distance_thresholds=list(a.distance_thresholds), iou_min_for_pose=a.iou_min_for_pose,
                  symmetric_classes=list(a.symmetric_classes), symmetry_axis=a.symmetry_axis, handle_class=a.handle_class)
    path = a.out or os.path.join(a.folder, "average_precision.json")
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("written", path)


if __name__ == "__main__":
    main()
