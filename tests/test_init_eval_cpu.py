"""CPU: the float64 twins of the batched eval-mode initialisation network and its validation numbers
(tests/init_train_twin.py::forward under eval(), tests/init_eval_twin.py) against the golden captured from the reference's
own modules; argument errors of the entry points of csrc/initnet_eval.hip (reported before any HIP call); the command
line's validation keys; and the conditions on the GPU tests' inputs with the table of fp32 floors."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import init_eval_twin as ev
import init_train_twin as tw
from helpers import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "init_eval.npz")


@pytest.fixture(scope="module")
def tables():
    return ev.grid_tables()


def test_cell_table_is_the_goldens(tables):
    """the cells' quaternions the golden's geodesic distances were taken with are what SO3Grid gives here"""
    gold = np.load(GOLDEN)
    for name, table in tables.items():
        if table is not None:
            stored = gold[f"grid_quats/{tw.CONFIGS[name]['orientation_grid_resolution']}"]
            assert stored.shape == (tw.CONFIGS[name]["cells"], 4) and np.array_equal(stored, table)
            assert np.abs(np.linalg.norm(table, axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("case", ev.CASES, ids=ev.case_key)
def test_twins_reproduce_the_reference(case, tables):
    """points, set features, output rows and the four validation sums of both batches: within 1e-9"""
    gold = np.load(GOLDEN)
    for which in (0, 1):
        cfg, _, x, t, feat, out = ev.batch(case, which, tables[case[0]])
        g = lambda k: gold[f"{ev.case_key(case)}/{which}/{k}"]
        assert np.array_equal(x, g("points"))
        assert np.abs(feat.numpy() - g("features")).max() <= 1e-9 * np.abs(g("features")).max()
        assert np.abs(out.numpy() - g("out")).max() <= 1e-9 * np.abs(g("out")).max()
        sums = ev.sums(out, cfg, t, tables[case[0]])
        assert np.allclose([sums[k] for k in ev.SUMS], g("sums"), rtol=1e-9, atol=0)
        assert (g("sums")[3] != 0) == bool(cfg["cells"])


def test_every_configuration_and_shape_of_the_issue_is_a_case():
    assert {c[0] for c in ev.CASES} == set(tw.CONFIGS)
    assert {c[1] for c in ev.CASES} >= {1, 37, 64, 65, 130}
    assert all(sorted(c[3]) in ([1, 3], [1, 2]) for c in ev.CASES)       # two batches of different N
    assert ("mug", 130, (2, 1)) in {(c[0], c[1], c[3]) for c in ev.CASES}


@pytest.mark.parametrize("case", ev.CASES, ids=ev.case_key)
def test_input_conditions_and_floors_table(case, tables):
    """batch() asserts the logit gap and the |q . q*| bound on both batches; the committed table holds these floors
    (python tests/init_eval_twin.py rewrites it): it sets the GPU bounds, so it may not lie above what this CPU measures
    by more than another CPU's last bits (a table BELOW it only tightens them)"""
    torch.set_num_threads(1)
    floor = ev.fp32_floor(case, tables[case[0]])
    stored = ev.load_floors()[ev.case_key(case)]
    print(ev.case_key(case), {k: f"{v:.2e} (table {stored[k]:.2e})" for k, v in floor.items()})
    assert sorted(stored) == sorted(floor)
    assert ("nll" in floor) == bool(tw.CONFIGS[case[0]]["cells"])
    for k, v in floor.items():
        assert 0 < stored[k] <= 1.5 * v and stored[k] <= 2e-6, k


@pytest.mark.parametrize("case", ev.TRAIN_CASES, ids=tw.case_key)
def test_train_metric_conditions_and_floor(case, tables):
    torch.set_num_threads(1)
    floor = ev.train_floor(case, tables[case[0]])
    stored = ev.load_floors()["train-" + tw.case_key(case)]
    print(tw.case_key(case), floor, stored)
    assert 0 < stored["geodesic"] <= 1.5 * floor["geodesic"] and stored["geodesic"] <= 2e-6


def test_metrics_twin_clip_and_first_maximum():
    """a prediction equal to the target gives a distance of 0, not NaN (|q . q*| a rounding above 1 is clipped); tied
    logits take the first cell"""
    cfg = tw.P16
    table = np.zeros((72, 4))
    table[:, 3] = 1.0
    table[5] = [0.6, 0.0, 0.0, 0.8]
    out = torch.zeros((2, tw.n_out(cfg)), dtype=torch.float64)
    out[0, cfg["latent_size"] + 4 + 5] = out[0, cfg["latent_size"] + 4 + 9] = 2.0          # cells 5 and 9 tie
    out[1, cfg["latent_size"] + 4 + 7] = 1.0
    t = {"position": np.zeros((2, 3)), "scale": np.zeros(2), "orientation": np.array([5, 7]),
         "quaternion": np.array([[0.6, 0.0, 0.0, 0.8], [0.0, 0.0, 0.0, 1.0 + 1e-12]])}
    v = ev.samples(out, cfg, t, table)
    assert v["geodesic"].tolist() == [0.0, 0.0]
    assert np.isclose(float(v["nll"][0]), np.log(2 * np.exp(2.0) + 70) - 2.0, rtol=1e-12)


def test_argument_errors_without_gpu():
    from sdfest_amd import _lib
    L = _lib.lib()
    err = lambda: L.sdfr_last_error()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)          # a non-NULL, 8-byte aligned pointer that is never dereferenced
    # the per-point layer on N sets: x, counts, N, M_capacity, cin, ldx, w, ldw, cvec, cvec_stride, scale, shift, resid,
    # y, ldy, cout, pool_resid, colmax
    layer = L.sdfr_pointnet_layer_batch
    ok = [q, q, 3, 130, 3, 3, q, 3, q, 0, q, q, None, q, 16, 16, 0, q, 0, None]
    bad = lambda **kw: [kw.get(n, v) for n, v in zip(("x", "counts", "N", "M", "cin", "ldx", "w", "ldw", "cvec", "stride",
                                                      "scale", "shift", "resid", "y", "ldy", "cout", "pool", "colmax",
                                                      "device", "stream"), ok)]
    assert layer(*bad(N=0)) == -1 and b"N=0" in err()
    assert layer(*bad(N=65536)) == -1
    assert layer(*bad(M=0)) == -1 and b"M_capacity=0" in err()           # a count array with a capacity of 0
    assert layer(*bad(N=40000, M=40000)) == -1 and b"2^30" in err()
    assert layer(*bad(ldx=2)) == -1 and layer(*bad(ldw=2)) == -1 and layer(*bad(ldy=8)) == -1 and layer(*bad(cout=0)) == -1
    assert layer(*bad(stride=8)) == -1 and b"cvec_stride" in err()
    for name in ("x", "w", "cvec", "scale", "shift", "colmax"):
        assert layer(*bad(**{name: None})) == -2, name
    assert layer(*bad(resid=q, y=None)) == -2 and b"a residual needs an output" in err()
    assert layer(*bad(pool=1)) == -2 and b"pool_resid needs a residual" in err()
    # N rows of a Linear: w, ldw, koff, x, ldx, k, bias, scale, shift, relu, y, ldy, cout, N
    rows = L.sdfr_linear_rows
    assert rows(q, 32, 0, q, 32, 32, q, q, q, 1, q, 16, 16, 0, 0, None) == -1 and b"N=0" in err()
    assert rows(q, 32, 0, q, 32, 32, q, q, q, 1, q, 16, 16, 65536, 0, None) == -1
    assert rows(q, 32, 16, q, 32, 32, q, q, q, 1, q, 16, 16, 3, 0, None) == -1        # koff + k > ldw
    assert rows(q, 32, 0, q, 16, 32, q, q, q, 1, q, 16, 16, 3, 0, None) == -1         # ldx < k
    assert rows(q, 32, 0, q, 32, 32, q, q, q, 1, q, 8, 16, 3, 0, None) == -1          # ldy < cout
    assert rows(None, 32, 0, q, 32, 32, q, q, q, 1, q, 16, 16, 3, 0, None) == -2
    assert rows(q, 32, 0, None, 32, 32, q, q, q, 1, q, 16, 16, 3, 0, None) == -2
    assert rows(q, 32, 0, q, 32, 32, q, q, q, 1, None, 16, 16, 3, 0, None) == -2
    assert rows(q, 32, 0, q, 32, 32, q, q, None, 1, q, 16, 16, 3, 0, None) == -2      # a scale without a shift
    # the validation numbers: out, N, ld_out, latent, n_cells, grid_quats, position, scale, quat, index, record, ws, bytes
    met = L.sdfr_pose_metrics
    big = 1 << 30
    assert L.sdfr_pose_metrics_workspace_bytes(0) == 0 and L.sdfr_pose_metrics_workspace_bytes(5) == 5 * 4 * 8
    assert met(q, 0, 79, 3, 72, q, q, q, q, q, q, q, big, 0, None) == -1 and b"N=0" in err()
    assert met(q, 4, 78, 3, 72, q, q, q, q, q, q, q, big, 0, None) == -1 and b"ld_out" in err()
    assert met(q, 4, 10, 3, 0, None, q, q, q, None, q, q, big, 0, None) == -1          # a quaternion row has L + 8
    assert met(q, 4, 79, 3, 72, None, q, q, q, q, q, q, big, 0, None) == -2 and b"grid_quats" in err()
    for i in (0, 6, 7, 8, 10, 11):
        args = [q, 4, 79, 3, 72, q, q, q, q, q, q, q, big, 0, None]
        args[i] = None
        assert met(*args) == -2, i
    assert met(q, 4, 79, 3, 72, q, q, q, q, q, ctypes.c_void_p(q.value + 4), q, big, 0, None) == -1 and b"aligned" in err()
    assert met(q, 4, 79, 3, 72, q, q, q, q, q, q, q, 4 * 4 * 8 - 1, 0, None) == -3 and b"workspace" in err()


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train_init_network as tool_module
    finally:
        sys.path.pop(0)
    return tool_module


def test_command_line_validation_keys():
    tool = _tool()
    block = {"width": 80, "size": 8}
    sets = {"camera": {"type": "SDFVAEViewDataset", "config_dict": block}}
    got = tool.validation_blocks({"validation_iteration": 2, "validation_datasets": sets})
    assert got == {"camera": block} and got["camera"] is not block           # (a copy: the tool edits it)
    with pytest.raises(NotImplementedError, match="NOCSDataset"):
        tool.validation_blocks({"validation_iteration": 2, "validation_datasets": dict(
            sets, real={"type": "NOCSDataset", "config_dict": {}})})


def test_command_line_without_validation_keys_takes_the_old_path():
    """no keys, the reference's default (an iteration and no sets), sets without an iteration: nothing to validate, and
    main() then calls fit exactly as before"""
    import inspect
    tool = _tool()
    sets = {"camera": {"type": "SDFVAEViewDataset", "config_dict": {}}}
    assert tool.validation_blocks({}) == {}
    assert tool.validation_blocks({"validation_iteration": 50000, "validation_datasets": {}}) == {}
    assert tool.validation_blocks({"validation_datasets": sets}) == {}
    src = inspect.getsource(tool.main)
    assert "if not validation:\n        trainer.fit(views, log_every=a.log_every)\n" in src
