"""CPU: the cases of tests/vae_train_cases.py are what the two GPU files take them for -- every hand-written edge
architecture and every default seed's random one meets the conditions under which a comparison of the VAE trainer with
its float64 twin means something, every seed finds its case within the sub-draws it has, and the edges together take
every path of the trainer's kernels that the list ``PATHS`` names."""
import os

import numpy as np
import pytest
import torch

import vae_train_cases as vc
import vae_train_twin as tw

SEEDS = range(int(os.environ.get("SDFR_FUZZ_SEEDS", "16")))


def assert_conditions(c):
    """the conditions of vae_train_cases.conditions, one assertion each"""
    from sdfest_amd.train import parameter_shapes
    what = f"{c.name} (sub-draw {c.sub}): {vc.describe(c.config)}"
    shapes = parameter_shapes(c.config)
    r = c.report
    print(f"{what}\n    branch margin {r.margin:.2e}, fp32 floor {r.floor:.2e}")
    assert c.config["sdf_size"] <= 20 and c.config["batch_size"] <= 5, what
    assert all(op["cout"] <= 40 for op in vc.train_ops(c.config)[0] if op["type"] == "conv"), what
    for phase in vc.PHASES:
        grads = c.reference[phase][1]
        assert sorted(grads) == sorted(k for k, _ in shapes), what
        assert all(grads[k].shape == tuple(s) for k, s in shapes), what
    assert not r.zero_gradients, f"{what}: gradients that are identically zero: {r.zero_gradients}"
    assert r.margin >= 1e-5, f"{what}: a value within {r.margin:.2e} of a branch"
    assert r.floor <= 1e-5, f"{what}: torch fp32 on the CPU is {r.floor:.2e} from float64"
    assert r.small_split, f"{what}: |x| < 0.1 everywhere or nowhere"
    assert r.clamp_split, f"{what}: the post phase's clamp mask is all true or all false"
    assert vc.accepted(r)


@pytest.mark.parametrize("name", list(vc.EDGES))
def test_edge_meets_the_conditions(name):
    assert_conditions(vc.edge(name))
    assert 10 <= len(vc.EDGES) <= 14


@pytest.mark.parametrize("seed", SEEDS)
def test_seed_finds_a_case_that_meets_the_conditions(seed):
    c = vc.case(seed)
    assert c is not None, f"seed {seed}: none of {vc.SUB_DRAWS} sub-draws meets the conditions"
    assert 0 <= c.sub < 20
    assert_conditions(c)


def test_edges_take_every_listed_path():
    took = {name: vc.paths(config, config["batch_size"]) for name, (config, _) in vc.EDGES.items()}
    for path in vc.PATHS:
        by = [name for name, t in took.items() if path in t]
        print(f"{path}: {', '.join(by)}")
        assert by, f"no edge architecture takes the path {path!r}"


def test_paths_are_read_from_the_shapes():
    """the path detector on the three architectures of tests/test_vae_train_gpu.py: what the issue found them to miss"""
    for config, N in ((tw.T16, 3), (tw.T8, 2)):
        took = vc.paths(config, N)
        assert took <= {"wgrad R % 32 != 0", "wgrad positions below one chunk", "wgrad positions between a chunk and a range",
                        "wgrad several ranges, short last", "wgrad N ranges < 16", "linear cout = 128",
                        "linear fin % 64 != 0 beyond 64", "pool tail no window covers"}, took   # T16 pools 7 -> 3
    ops, features = vc.train_ops(tw.T16)
    assert features == 12 and [op["type"] for op in ops] == ["conv", "conv", "pool", "linear", "linear", "linear", "conv",
                                                            "resize", "conv", "resize", "conv", "resize"]
    assert [op["gin"] for op in ops[:4]] == [False, True, True, True] and ops[2]["relu"] is False and ops[1]["relu"]
    assert (ops[0]["n"], ops[0]["m"], ops[2]["m"], ops[-1]["n"], ops[-1]["m"]) == (16, 7, 3, 10, 16)


def test_traced_forward_is_the_twins_forward():
    """branch_margin reads the activations of a forward of its own: the same bits as vae_train_twin.forward"""
    for name in ("pool_first_k1_relu", "resize_from_1_last_relu", "linear_127_128_129", "relu_first"):
        c = vc.edge(name)
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in c.state.items()}
        x, eps = torch.tensor(c.x, dtype=torch.float64), torch.tensor(c.eps, dtype=torch.float64)
        with torch.no_grad():
            ref = tw.forward(params, c.config, x, eps)
            got, relus, pools = vc.traced_forward(params, c.config, x, eps)
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), name
        layers = [i["type"].rsplit(".", 1)[-1] for i in c.config["encoder"]["layer_infos"]]
        dec = c.config["decoder"]
        assert len(relus) == layers.count("ReLU") + len(dec["fc_layers"]) + sum(l["relu"] for l in dec["conv_layers"])
        assert len(pools) == layers.count("MaxPool3d")


def test_branch_margin_sees_each_branch():
    """a value moved next to a branch lowers the margin to its distance: a ReLU input, a pool window's runner-up, |x| at
    0.1 and at tsdf, |recon| at tsdf"""
    config, state = tw.T16, tw.random_state(tw.T16, 11)
    x = tw.blobs_at(16, (0, 1))
    eps = np.zeros((2, 3), np.float32)
    base = vc.branch_margin(config, state, x, eps)
    assert 0 < base < 1
    top = np.abs(x).max()
    for level in (0.1, 0.3):
        moved = x.copy()
        moved[0, 0, 3, 4, 5] = level + 1e-7
        got = vc.branch_margin(dict(config, tsdf=0.3), state, moved, eps)
        assert got <= 2e-7 / top, (level, got)
    assert vc.branch_margin(dict(config, tsdf=False), state, x, eps) >= base
    # |recon| next to tsdf: with tsdf = 10 nothing of x is clamped, and the last layer's bias (no ReLU; the resize behind it
    # passes a constant on) moved so that one reconstruction value is 10 - 1e-6
    params = {k: torch.tensor(v, dtype=torch.float64) for k, v in state.items()}
    x64, e64 = torch.tensor(x, dtype=torch.float64), torch.tensor(eps, dtype=torch.float64)
    with torch.no_grad():
        (_, _, _, recon), relus, pools = vc.traced_forward(params, config, x64, e64)
    shifted = dict(state)
    shifted["decoder._conv_layers.2.bias"] = state["decoder._conv_layers.2.bias"].astype(np.float64) \
        + (10.0 - 1e-6 - float(recon[1, 0, 8, 9, 10]))
    assert vc.branch_margin(dict(config, tsdf=10.0), shifted, x, eps) <= 2e-7
    assert vc.branch_margin(dict(config, tsdf=10.0), state, x, eps) > 2e-7
    # a ReLU input next to zero: the first encoder bias moved so that one pre-activation is 1e-9
    pre = relus[0]
    shifted = dict(state)
    shifted["encoder._features.0.bias"] = state["encoder._features.0.bias"].astype(np.float64)
    shifted["encoder._features.0.bias"][1] -= float(pre[0, 1, 2, 2, 2]) - 1e-9
    assert vc.branch_margin(config, shifted, x, eps) <= 1e-7 < base
    # the runner-up of a pool window: the gap of the closest window is what the margin reports when nothing else is closer
    h, k, s = pools[0]
    win = h.unfold(2, k, s).unfold(3, k, s).unfold(4, k, s).reshape(-1, k ** 3)
    two = torch.topk(win, 2, dim=1).values
    gaps = (two[:, 0] - two[:, 1])
    assert base <= float(gaps[gaps > 0].min() / h.abs().max())
