#!/usr/bin/env python3
"""Preprocess one split of a NOCS root directory on the GPU (what the first ``NOCSDataset`` construction does) and
print the rate, the share of skipped objects and the per-category counts.

Usage:  python tools/preprocess_nocs.py --root_dir /data/nocs --split real_train [--seed 0] [--batch 64]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir", required=True)
    ap.add_argument("--split", required=True, choices=["camera_train", "camera_val", "real_train", "real_test"])
    ap.add_argument("--seed", type=int, default=0, help="key of the RANSAC's sample stream")
    ap.add_argument("--batch", type=int, default=64, help="frames per fit launch")
    args = ap.parse_args()
    from sdfest_amd import NOCSDataset
    ds = NOCSDataset({"root_dir": args.root_dir, "split": args.split, "seed": args.seed, "preprocess_batch": args.batch})
    stats = ds.preprocess_stats
    if stats is None:
        print(f"{args.split} was preprocessed before: {len(ds)} samples in "
              f"{os.path.join(args.root_dir, 'sdfest_pre', args.split)}")
        return
    seen = stats["objects"] + stats["skipped"]
    print(json.dumps({"split": args.split, "frames": stats["frames"], "objects": stats["objects"],
                      "skipped": stats["skipped"], "skipped_share": stats["skipped"] / seen if seen else 0.0,
                      "seconds": stats["seconds"], "objects_per_s": stats["objects"] / max(stats["seconds"], 1e-9),
                      "categories": stats["categories"]}))


if __name__ == "__main__":
    main()
