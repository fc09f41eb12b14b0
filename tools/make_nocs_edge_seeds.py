#!/usr/bin/env python3
"""Choose the seeds of tests/nocs_edges.py's seeded cases and write them to tests/golden/nocs_edge_seeds.json.

  sweep       one seed per slot (tests/nocs_edges.py::sweep_slot): the first of at most 20 tried in order whose case
              passes the margins of tools/make_nocs_goldens.py, recomputed with tests/nocs_twin.py
  pose_error  per point count (5, 6) the first seed whose winner keeps a single inlier that is not point 0, so that the
              FINAL fit has no variance

Nothing but the twin and the builders is imported; the file is reproduced byte for byte.

Usage:  python tools/make_nocs_edge_seeds.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nocs_edges as ne      # noqa: E402
import nocs_twin as tw       # noqa: E402


def seeds():
    return {"pose_error": {str(n): ne.find_pose_error_seed(n) for n in (5, 6)},
            "sweep": [ne.find_sweep_seed(i) for i in range(ne.SWEEP_SLOTS)]}


def text(s):
    return json.dumps(s, indent=1, sort_keys=True) + "\n"


def main():
    s = seeds()
    for i, seed in enumerate(s["sweep"]):
        c = ne.sweep_case(i, seed)
        o = tw.ransac(c["source"], c["target"], c["draws"])
        print(f"sweep{i:02d}: seed {seed} (try {seed - ne.sweep_slot(i)[4]}) N {len(c['source'])} {c['source'].dtype} "
              f"status {o['status']} ran {o['iterations_run']} winner {o['best_iteration']} "
              f"inliers {len(o['inlier_idx'])}")
    print("pose_error:", s["pose_error"])
    path = os.path.join(ROOT, "tests", "golden", ne.SEEDS_FILE)
    with open(path, "w") as f:
        f.write(text(s))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
