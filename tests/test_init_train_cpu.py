"""CPU: the float64 twin of the initialisation network's training iteration (tests/init_train_twin.py) against the golden
captured from the reference's own modules; the parameter layout against the library's; argument errors of every entry
point of include/sdfr.h group 11 (reported before any HIP call); the host-side pieces of sdfest_amd.init_train; and the
conditions on the GPU tests' inputs (Accuracy): branch margins, null tensors, the fp32 floors and their
table."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import init_train_twin as tw
from helpers import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "init_train.npz")
GOLDEN_CASES = {"mug": ("mug", 4, 64, 26, 3.0), "plain": ("Q16", 3, 130, 0, 0.0)}     # tools/make_init_train_goldens.py
EVERY = 97


@pytest.mark.parametrize("tag", list(GOLDEN_CASES))
def test_twin_reproduces_the_reference(tag):
    """terms, output rows, every parameter's gradient (maximum, norm, every 97th element) and the running statistics
    after the step: within 1e-9 of each tensor's maximum (a null tensor: of its layer's weight gradient's)"""
    gold = np.load(GOLDEN)
    cfg, state, x, t = tw.case_setup(GOLDEN_CASES[tag])
    terms, grads, out, stats = tw.Twin(cfg, state).loss_and_grad(x, t)
    keys = [str(k) for k in gold[f"{tag}/keys"]]
    assert keys == [k for k, _ in tw.parameter_shapes(cfg)]                  # the reference's parameters() order
    assert np.allclose([terms[k] for k in tw.TERMS], gold[f"{tag}/terms"], rtol=1e-9, atol=0)
    assert np.abs(out - gold[f"{tag}/out"]).max() <= 1e-9 * np.abs(out).max()
    nulls = tw.null_tensors(grads)
    for k in keys:
        g, top = grads[k].ravel(), gold[f"{tag}/grad_max/{k}"]
        if k in nulls:       # mathematically zero: both sides hold rounding noise, small against the layer's weight gradient
            scale = gold[f"{tag}/grad_max/{k.rsplit('.', 1)[0]}.weight"]
            assert np.abs(g).max() <= 1e-9 * scale and top <= 1e-9 * scale, k
            continue
        assert abs(np.abs(g).max() - top) <= 1e-9 * top, k
        assert abs(np.linalg.norm(g) - gold[f"{tag}/grad_norm/{k}"]) <= 1e-9 * top * np.sqrt(g.size), k
        assert np.abs(g[::EVERY] - gold[f"{tag}/grad_every/{k}"]).max() <= 1e-9 * top, k
    assert sorted(stats) == sorted(k[len(tag) + 6:] for k in gold.files if k.startswith(f"{tag}/stat/"))
    for k, v in stats.items():
        assert np.abs(v - gold[f"{tag}/stat/{k}"]).max() <= 1e-9 * np.abs(v).max(), k


def _create(L, cfg, device=0):
    arr = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    bb, hd = cfg["backbone"], cfg["head"]
    a, b = arr(bb["mlp_out_sizes"]), arr(hd["mlp_out_sizes"])
    h = ctypes.c_void_p()
    rc = L.sdfr_pose_trainer_create(bb["in_size"], len(a), a.ctypes.data_as(ctypes.c_void_p), int(bb["batchnorm"]),
                                    int(bb["dense"]), int(bb["residual"]), len(b), b.ctypes.data_as(ctypes.c_void_p),
                                    int(hd["batchnorm"]), cfg["latent_size"], cfg["cells"], device, ctypes.byref(h))
    return rc, h


@pytest.mark.parametrize("name", list(tw.CONFIGS))
def test_parameter_layout_is_the_librarys(name):
    from sdfest_amd import _lib, init_train
    L = _lib.lib()
    cfg = tw.CONFIGS[name]
    rc, h = _create(L, cfg)
    assert rc == 0
    shapes = tw.parameter_shapes(cfg)
    assert L.sdfr_pose_trainer_param_count(h) == sum(int(np.prod(s)) for _, s in shapes)
    assert L.sdfr_pose_trainer_stat_count(h) == 2 * sum(c for _, c in tw.stat_shapes(cfg))
    assert L.sdfr_pose_trainer_output_size(h) == tw.n_out(cfg)
    checked = init_train.check_config(tw.train_config(cfg))
    assert init_train.parameter_shapes(checked) == [(k, tuple(s)) for k, s in shapes]
    assert init_train.stat_shapes(checked) == tw.stat_shapes(cfg) and init_train.num_cells(checked) == cfg["cells"]
    assert L.sdfr_pose_trainer_tape_bytes(h, 4, 37) > 0 and L.sdfr_pose_trainer_workspace_bytes(h, 4, 37) > 0
    L.sdfr_pose_trainer_destroy(h)


def test_argument_errors_without_gpu():
    from sdfest_amd import _lib
    L = _lib.lib()
    err = lambda: L.sdfr_last_error()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)          # a non-NULL, 8-byte aligned pointer that is never dereferenced
    big = 1 << 40
    two = np.array([16, 16], np.int32).ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_void_p()
    ref = ctypes.byref(h)
    # create
    assert L.sdfr_pose_trainer_create(3, 2, two, 1, 0, 0, 2, two, 1, 3, 0, 0, None) == -2
    assert L.sdfr_pose_trainer_create(3, 2, None, 1, 0, 0, 2, two, 1, 3, 0, 0, ref) == -2
    assert L.sdfr_pose_trainer_create(0, 2, two, 1, 0, 0, 2, two, 1, 3, 0, 0, ref) == -1 and b"in_size" in err()
    assert L.sdfr_pose_trainer_create(3, 0, two, 1, 0, 0, 2, two, 1, 3, 0, 0, ref) == -1 and b"n_backbone" in err()
    assert L.sdfr_pose_trainer_create(3, 2, two, 1, 0, 0, 0, two, 1, 3, 0, 0, ref) == -1 and b"n_head" in err()
    assert L.sdfr_pose_trainer_create(3, 2, two, 1, 0, 0, 2, two, 1, 0, 0, 0, ref) == -1 and b"latent" in err()
    assert L.sdfr_pose_trainer_create(3, 2, two, 1, 0, 0, 2, two, 1, 3, -1, 0, ref) == -1 and b"n_cells" in err()
    bad = np.array([16, 0], np.int32).ctypes.data_as(ctypes.c_void_p)
    assert L.sdfr_pose_trainer_create(3, 2, bad, 1, 0, 0, 2, two, 1, 3, 0, 0, ref) == -1 and b"width 0" in err()
    assert L.sdfr_pose_trainer_create(32, 2, two, 1, 1, 1, 2, two, 1, 3, 0, 0, ref) == -1 and b"residual" in err()
    assert not h.value
    # the sizes refuse what the calls refuse
    for f in (L.sdfr_pose_trainer_param_count, L.sdfr_pose_trainer_stat_count, L.sdfr_pose_trainer_output_size):
        assert f(None) == 0
    rc, h = _create(L, tw.P16)
    assert rc == 0
    for f in (L.sdfr_pose_trainer_tape_bytes, L.sdfr_pose_trainer_workspace_bytes):
        assert f(None, 4, 37) == 0 and f(h, 0, 37) == 0 and f(h, 4, 0) == 0 and f(h, 1, 37) == 0 and f(h, 70000, 2) == 0
        assert f(h, 65535, 65535) == 0
    # forward
    fwd = L.sdfr_pose_trainer_forward
    assert fwd(None, q, q, q, 4, 37, 0, q, q, big, q, big, None) == -2
    assert fwd(h, q, q, q, 1, 37, 0, q, q, big, q, big, None) == -1 and b"N >= 2" in err()       # the head's BatchNorm
    assert fwd(h, q, q, q, 4, 0, 0, q, q, big, q, big, None) == -1 and b"M" in err()
    assert fwd(h, None, q, q, 4, 37, 0, q, q, big, q, big, None) == -2
    assert fwd(h, q, None, q, 4, 37, 1, q, q, big, q, big, None) == -2 and b"statistics" in err()
    assert fwd(h, q, q, q, 4, 37, 0, q, q, big, ctypes.c_void_p(q.value + 4), big, None) == -1 and b"aligned" in err()
    assert fwd(h, q, q, q, 4, 37, 0, q, q, 16, q, big, None) == -3 and b"tape" in err()
    assert fwd(h, q, q, q, 4, 37, 0, q, q, big, q, 16, None) == -3 and b"workspace" in err()
    # loss
    loss = L.sdfr_pose_trainer_loss
    assert loss(None, q, q, q, q, q, None, 4, 1.0, 1.0, 1.0, 1.0, q, q, q, big, None) == -2
    assert loss(h, q, q, q, q, q, None, 0, 1.0, 1.0, 1.0, 1.0, q, q, q, big, None) == -1
    assert loss(h, q, q, q, q, None, q, 4, 1.0, 1.0, 1.0, 1.0, q, q, q, big, None) == -2 and b"class index" in err()
    assert loss(h, q, q, q, q, q, None, 4, 1.0, 1.0, 1.0, 1.0, None, q, q, big, None) == -2
    assert loss(h, q, q, q, q, q, None, 4, 1.0, 1.0, 1.0, 1.0, q, q, q, 16, None) == -3
    rc, hq = _create(L, tw.Q16)
    assert rc == 0
    assert loss(hq, q, q, q, q, q, None, 4, 1.0, 1.0, 1.0, 1.0, q, q, q, big, None) == -2 and b"quaternion" in err()
    # backward
    bwd = L.sdfr_pose_trainer_backward
    assert bwd(None, q, q, 4, 37, q, q, q, q, big, None) == -2
    assert bwd(h, q, q, 1, 37, q, q, q, q, big, None) == -1
    assert bwd(h, q, q, 4, 37, q, None, q, q, big, None) == -2
    assert bwd(h, q, q, 4, 37, q, q, q, ctypes.c_void_p(q.value + 4), big, None) == -1
    assert bwd(h, q, q, 4, 37, q, q, q, q, 16, None) == -3 and b"workspace" in err()
    assert bwd(hq, q, q, 1, 37, q, q, q, q, 16, None) == -3          # no BatchNorm: N = 1 is a shape, not an error
    L.sdfr_pose_trainer_destroy(h)
    L.sdfr_pose_trainer_destroy(hq)
    L.sdfr_pose_trainer_destroy(None)


def test_config_checks_and_initial_state():
    from sdfest_amd import init_train
    config = tw.train_config(tw.P16)
    for key in init_train.WEIGHTS:
        with pytest.raises(KeyError, match=key):
            init_train.check_config({k: v for k, v in config.items() if k != key})
    with pytest.raises(NotImplementedError, match="backbone_type"):
        init_train.check_config(dict(config, backbone_type="IterativePointNet"))
    with pytest.raises(NotImplementedError, match="head_type"):
        init_train.check_config(dict(config, head_type="Other"))
    checked = init_train.check_config(config)
    assert checked["head"]["orientation_repr"] == "discretized" and checked["head"]["orientation_grid_resolution"] == 0
    assert "orientation_repr" not in config["head"]                   # the caller's dictionaries are left alone
    a, b, c = (init_train.initial_state(config, s) for s in (0, 0, 1))
    assert list(a)[:2] == ["_backbone._linear_layers.0.weight", "_backbone._linear_layers.0.bias"]
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["_head._final_layer.weight"],
                                                                       c["_head._final_layer.weight"])
    for key, shape in init_train.parameter_shapes(checked):
        t = a[key]
        assert tuple(t.shape) == shape and t.dtype == torch.float32
        if "_bn_layers" in key:
            assert torch.all(t == (1.0 if key.endswith("weight") else 0.0))
        elif key.endswith("weight"):                                   # U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
            bound = 1.0 / np.sqrt(shape[1])
            assert t.abs().max() <= bound and a[key[:-6] + "bias"].abs().max() <= bound
            assert t.numel() < 64 or t.abs().max() > 0.8 * bound
    for prefix, n in init_train.stat_shapes(checked):
        assert torch.all(a[prefix + ".running_mean"] == 0) and torch.all(a[prefix + ".running_var"] == 1)
        assert a[prefix + ".num_batches_tracked"].dtype == torch.int64 and a[prefix + ".running_var"].shape == (n,)
    # what torch's own modules hold by default, key for key
    lin, bn = torch.nn.Linear(3, 16), torch.nn.BatchNorm1d(16)
    assert lin.weight.abs().max() <= 1 / np.sqrt(3) and list(bn.state_dict()) == [
        "weight", "bias", "running_mean", "running_var", "num_batches_tracked"]


def test_checkpoint_file_round_trips(tmp_path):
    from sdfest_amd import init_train
    ck = {"params": torch.arange(5.0), "stats": torch.ones(4), "batches_tracked": 7, "exp_avg": torch.zeros(5),
          "exp_avg_sq": torch.full((5,), 2.0), "adam_step": 7, "iteration": 7, "seed": 3,
          "config": tw.train_config(tw.P16), "keys": ["a", "b"]}
    path = str(tmp_path / "t.ckpt")
    init_train.write_checkpoint(path, ck)
    back = init_train.read_checkpoint(path)
    assert sorted(back) == sorted(ck)
    assert all(torch.equal(back[k], v) if isinstance(v, torch.Tensor) else back[k] == v for k, v in ck.items())
    init_train.write_checkpoint(path, {k: v for k, v in ck.items() if k != "stats"})
    with pytest.raises(ValueError, match="stats"):
        init_train.read_checkpoint(path)


def test_command_line_help_and_dataset_types():
    tool = os.path.join(ROOT, "tools", "train_init_network.py")
    done = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "--config" in done.stdout and "--out" in done.stdout
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train_init_network as tool_module
    finally:
        sys.path.pop(0)
    block = {"width": 80}
    datasets = {"a": {"type": "SDFVAEViewDataset", "probability": 1.0, "config_dict": block},
                "b": {"type": "NOCSDataset", "probability": 0.0}}
    assert tool_module.dataset_block({"datasets": datasets}) == block
    datasets["b"]["probability"] = 0.5
    with pytest.raises(NotImplementedError, match="NOCSDataset"):
        tool_module.dataset_block({"datasets": datasets})


@pytest.mark.parametrize("case", tw.CASES, ids=tw.case_key)
def test_input_conditions_of_the_gpu_cases(case):
    """the branch margin of the case's inputs is >= 1e-5; its null tensors are the Linear biases in front of a BatchNorm;
    torch fp32 on the CPU against the twin (the floor) stays <= 1e-4 on the gradients and below the GPU tests' absolute
    bound on the null tensors; the committed table holds these floors (python tests/init_train_twin.py rewrites it)"""
    cfg, state, x, t = tw.case_setup(case)
    if cfg["backbone"]["batchnorm"]:
        assert case[1] >= 4
    assert tw.branch_margin(cfg, state, x, t) >= 1e-5
    _, grads, _, _ = tw.Twin(cfg, state).loss_and_grad(x, t)
    nulls = tw.null_tensors(grads)
    part = lambda k: cfg["backbone" if k.startswith("_backbone") else "head"]
    expected = {k for k, _ in tw.parameter_shapes(cfg) if "_linear_layers" in k and k.endswith(".bias") and
                part(k)["batchnorm"]}
    assert expected <= set(nulls) and all(k.endswith(".bias") for k in nulls)   # (and whatever else a later
    # batch normalisation removes, e.g. the last backbone BatchNorm's bias of B16 when every pooled maximum is positive)
    torch.set_num_threads(1)
    floor = tw.fp32_floor(case)
    stored = tw.load_floors()[tw.case_key(case)]
    print(tw.case_key(case), {k: f"{v:.2e} (table {stored[k]:.2e})" for k, v in floor.items()})
    assert floor["grad"] <= 1e-4 and stored["grad"] <= 1e-4
    assert floor["null"] <= 4.2e-5 and stored["null"] <= 4.2e-5     # (the GPU tests allow ten times this figure)
    for k, v in floor.items():      # the table sets the GPU bounds: it may not lie above what this CPU measures by more
        assert stored[k] <= 1.5 * v, k     # than another CPU's last bits (a table BELOW it only tightens the GPU bounds)


def test_trajectory_floor_is_the_tables():
    torch.set_num_threads(1)
    floor, stored = tw.trajectory_floor(), tw.load_floors()["trajectory"]["total"]
    print(f"trajectory floor {floor:.2e} (table {stored:.2e})")
    assert stored <= 1.5 * floor
