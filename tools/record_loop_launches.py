"""Writes tests/golden/loop_launch_sequences.json: the C ABI calls that one run of every loop form issues
(tests/loop_launches.py: the cases and the recorder; tests/test_loop_launches_gpu.py compares against the file).

A recorded result of this repository's own code, on a GPU.  Record it on the commit whose launch sequences are to be
kept, BEFORE changing the loops' host code:

    python tools/record_loop_launches.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import loop_launches as LL
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=LL.FIXTURE_PATH)
    out = ap.parse_args().out
    decoders = {}
    logs = {case: LL.record_case(kind, kw, decoders) for case, (kind, kw) in LL.cases().items()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:       # one call per line: a changed launch shows as a changed line
        f.write("{\n")
        for i, (case, log) in enumerate(sorted(logs.items())):
            f.write(f" {json.dumps(case)}: [\n")
            f.write(",\n".join("  " + json.dumps(call) for call in log))
            f.write("\n ]" + ("," if i + 1 < len(logs) else "") + "\n")
        f.write("}\n")
    for case, log in logs.items():
        print(f"{case}: {len(log)} calls")


if __name__ == "__main__":
    main()
