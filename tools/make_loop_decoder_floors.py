"""Writes tests/golden/loop_decoder_floors.json: for every decoder of tests/loop_decoders.py and each of its scenes, the
distance per parameter group between the float32 and the float64 statement of the loop's first gradient -- what the
number format alone costs there.  tests/test_loop_decoders_gpu.py bounds the kernels by max(1e-4, 10 x floor);
tests/test_loop_decoders_cpu.py recomputes the floors and requires the committed ones within a factor of 2.

A recorded result of this repository's own code: everything is computed by the helper (CPU only, a few seconds).

    python tools/make_loop_decoder_floors.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import loop_decoders as D
    floors = {name: {which: [float(f"{x:.3e}") for x in D.compute_floor(name, which)] for which in D.SCENES}
              for name in D.NAMES}
    with open(D.FLOORS_PATH, "w") as f:
        json.dump(floors, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, per in floors.items():
        print(name, per)


if __name__ == "__main__":
    main()
