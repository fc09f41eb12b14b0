"""Writes tests/golden/shading_floors.json: per scene of tests/shading_twin.py (TWIN_SCENES), the largest angle in radians
between the twin's normals evaluated in float32 and in float64 on the scene's golden depth, over the hit pixels the
comparison keeps (shading_twin.excluded: not within 1e-3 grid units of a cell face, |g| not below 1e-3 of the largest)
-- what float32 arithmetic alone costs, on the CPU.  tests/test_shading_gpu.py holds the GPU to
max(1e-4 rad, 10 x this floor).  The convention of decoder_jvp_floors.json.

    python tools/make_shading_floors.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import shading_twin as T          # noqa: E402
from helpers import load_render_case   # noqa: E402


def scene_floor(name):
    c = load_render_case(name)
    args = (c["sdf"], c["p"], c["q"], c["inv_scale"], c["cx"], c["cy"], c["fx"], c["fy"])
    depth = c["depth"].astype(np.float32)
    n64, info = T.normals(depth, *args, dtype=np.float64)
    n32, _ = T.normals(depth, *args, dtype=np.float32)
    keep = info["hit"] & ~T.excluded(info)
    share = float(T.excluded(info).sum()) / max(int(info["hit"].sum()), 1)
    return (float(np.max(T.angles(n32, n64)[keep])) if keep.any() else 0.0), share


def main():
    floors = {}
    for name in T.TWIN_SCENES:
        floor, share = scene_floor(name)
        floors[name] = float(f"{floor:.3e}")
        print(f"{name:28s} floor {floor:.3e} rad   left out {100 * share:.2f} %")
    with open(T.FLOORS, "w") as f:
        json.dump(floors, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", T.FLOORS)


if __name__ == "__main__":
    main()
