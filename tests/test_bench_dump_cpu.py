"""CPU: bench.dump_outputs -- what the last timed step returned, as float32 .npy files below 64 MB in all, the depth
images as a seeded sample of whole views that depends on the shapes alone (two builds given the same arguments dump
the same views).  Driven with a stand-in plan of CPU tensors whose view b is filled with b."""
import os
from types import SimpleNamespace

import numpy as np
import torch

import bench

NAMES = ["depth_sample", "grad_inv_scale", "grad_position", "grad_quaternion", "grad_sdf"]


def fake_plan(B, H, W):
    return SimpleNamespace(depth=torch.arange(B, dtype=torch.float32)[:, None, None].expand(B, H, W).contiguous(),
                           g_sdf=torch.randn(64, 64, 64), g_pos=torch.randn(B, 3), g_quat=torch.randn(B, 4),
                           g_inv_scale=torch.randn(B))


def load(d):
    assert sorted(os.listdir(d)) == [n + ".npy" for n in NAMES]
    out = {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}
    assert all(a.dtype == np.float32 for a in out.values())
    assert sum(os.path.getsize(os.path.join(d, n + ".npy")) for n in NAMES) <= 64e6
    return out


def test_a_default_step_dumps_a_fixed_sample_of_whole_views(tmp_path):
    plan = fake_plan(256, 480, 640)
    assert bench.dump_outputs(str(tmp_path / "a"), plan) == NAMES
    bench.dump_outputs(str(tmp_path / "b"), plan)
    a, b = load(tmp_path / "a"), load(tmp_path / "b")
    d = a["depth_sample"]
    assert d.shape == (40, 480, 640)
    views = d[:, 0, 0].astype(int)
    assert (d == views[:, None, None]).all()                         # whole views ...
    assert (np.diff(views) > 0).all() and views[-1] - views[0] > 128  # ... in view order, spread over the batch
    for n in NAMES:
        assert np.array_equal(a[n], b[n])
    assert np.array_equal(a["grad_sdf"], plan.g_sdf.numpy()) and np.array_equal(a["grad_position"], plan.g_pos.numpy())
    assert np.array_equal(a["grad_quaternion"], plan.g_quat.numpy())
    assert np.array_equal(a["grad_inv_scale"], plan.g_inv_scale.numpy())


def test_a_small_step_dumps_every_view(tmp_path):
    plan = fake_plan(6, 24, 32)
    bench.dump_outputs(str(tmp_path), plan)
    assert np.array_equal(load(tmp_path)["depth_sample"], plan.depth.numpy())


def test_a_view_larger_than_the_budget_is_sampled_by_pixel(tmp_path):
    plan = fake_plan(2, 3600, 4000)
    plan.depth[:] = torch.arange(3600 * 4000, dtype=torch.float32).view(3600, 4000)    # (exact in float32)
    bench.dump_outputs(str(tmp_path), plan)
    d = load(tmp_path)["depth_sample"]
    assert d.shape == (1, bench.DUMP_DEPTH_BYTES // 4)
    assert (np.diff(d[0]) > 0).all()                                 # distinct pixels of one view, in order
