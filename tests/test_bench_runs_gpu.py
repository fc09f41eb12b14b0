"""GPU: bench.py's two kinds of run, on a small workload.  A plain run measures the headline alone -- exactly --steps
timed steps, one line with `ms_per_step` -- and `--dump-outputs DIR` writes what its last timed step returned, the same
from run to run; `--full` adds the parity report, the CPU port, the clock telemetry and the side configurations."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, W, H, STEPS = 16, 320, 240, 7
SMALL = ["--gpus", "1", "--steps", str(STEPS), "--warmup", "2", "--batch", str(B), "--width", str(W), "--height", str(H),
         "--prewarm-ms", "0"]
MOVED = {"parity", "grad_max_abs_err", "cpu_baseline", "speedup_vs_cpu", "configs", "gpu_telemetry"}


def bench(*extra, timeout=300):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], capture_output=True,
                         text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


def load(d):
    names = ["depth_sample", "grad_inv_scale", "grad_position", "grad_quaternion", "grad_sdf"]
    assert sorted(os.listdir(d)) == [n + ".npy" for n in names]
    return {n: np.load(os.path.join(d, n + ".npy")) for n in names}


def test_plain_run_is_the_headline_and_dumps_its_last_step(tmp_path):
    line = bench("--dump-outputs", str(tmp_path / "a"))
    assert line["unit"] == "renders/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["n_gpus"] == 1 and line["steps"] == STEPS and line["value"] > 0
    assert abs(B / (line["ms_per_step"] * 1e-3) / line["value"] - 1) < 0.01
    assert line["step_ms_events"]["n"] == 2                   # events on every 4th of the 7 timed steps: 0 and 4
    assert not MOVED & set(line), MOVED & set(line)
    a = load(tmp_path / "a")
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["depth_sample"].shape == (B, H, W) and a["grad_sdf"].shape == (64, 64, 64)
    assert a["grad_position"].shape == (B, 3) and a["grad_quaternion"].shape == (B, 4) and a["grad_inv_scale"].shape == (B,)
    assert int((a["depth_sample"] > 0).sum()) == line["config"]["hit_pixels_rank0"] > 1000
    assert np.abs(a["grad_sdf"]).max() > 0 and np.abs(a["grad_position"]).max() > 0
    # the same inputs in a second process: depth bit for bit, the gradients up to the order of their float sums
    bench("--dump-outputs", str(tmp_path / "b"))
    b = load(tmp_path / "b")
    assert np.array_equal(a["depth_sample"], b["depth_sample"])
    for n in ("grad_sdf", "grad_position", "grad_quaternion", "grad_inv_scale"):
        assert np.max(np.abs(a[n] - b[n])) <= 1e-3 * np.max(np.abs(a[n])), n


def test_full_run_adds_what_the_plain_run_leaves_out():
    line = bench("--full", timeout=600)
    assert line["steps"] == STEPS and line["value"] > 0 and line["ms_per_step"] > 0
    assert MOVED <= set(line), MOVED - set(line)
    assert line["parity"]["views"] == B and line["parity"]["grad_sdf"]["max_err_over_max"] < 1e-4
    assert line["cpu_baseline"]["value"] > 0 and line["configs"]["C1"]["renders_per_s"] > 0
