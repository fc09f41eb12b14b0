"""GPU: the initialisation network's trainer (sdfest_amd.SDFPoseNetTrainer over csrc/initnet_train.hip; the C entry points
where the cell count is none an SO3 grid has) on the hand-written edges of tests/init_train_cases.py against the float64
twin (tests/init_train_twin.py) -- the comparison of test_init_train_gpu.py at the shapes its six architectures never
reach: reduction lengths, column counts and record widths just past a 64-wide tile, 1024 and 1025 rows, sets of 1, 2, 3,
31 and 33 points, tiles spanning three samples, every link form of the host walk (a residual link from the points, one
layer, dense without residual, residual never taken), BatchNorm in one part only, heads of one and three layers and of
300 columns, N = 1 and N = 2, latent sizes 1, 65 and 70, 5 and 130 cells, 1, 4 and 70 input columns.
tests/test_init_train_cases_cpu.py asserts that the edges take each of those paths and that no branch, dead layer or
stray null tensor makes a case vacuous.

Bounds (Accuracy; tests/golden/init_train_case_floors.json holds the floors, the CPU file re-derives
them): 10 x max(the case's own fp32 floor, one fp32 ulp = 2^-23) -- the floor is how far torch fp32 on the CPU lies from
float64 on the case's inputs, 10 x the project's margin for another summation order, and the clamp is there because a
five-operation net can land below an ulp on the CPU by luck while no fp32 result owes more than that -- of each gradient
tensor's float64 maximum, of the output rows' and the running statistics' maximum, and relative + 1e-6 on the loss
terms; null tensors within 4.2e-4 of their layer's weight gradient."""
import numpy as np
import pytest
import torch

import init_train_cases as ic
import init_train_twin as tw

pytestmark = pytest.mark.gpu

MARGIN = 10.0
ULP = 2.0 ** -23
NULL_BOUND = 4.2e-4
# one edge per link form, for the inference network on what training wrote: a residual link from the points (one layer,
# no BatchNorm), dense without residual, dense + residual under BatchNorm (into a dense link and into the last layer),
# no link at all on 70 input columns
INFERENCE = ("points_residual_one_layer", "dense_plain_50_100_67", "in_1_dense_residual_m3", "in_70_backbone_bn")


def device_inputs(x, t):
    return torch.tensor(x, dtype=torch.float32, device="cuda"), {k: torch.tensor(v, device="cuda") for k, v in t.items()}


def new_trainer(c):
    from sdfest_amd import SDFPoseNetTrainer
    return SDFPoseNetTrainer(tw.train_config(c.cfg), c.state)


def run(c, trainer=None, x=None, t=None):
    """loss_and_grad of the case (or of other inputs) with the gradients cloned: they are views of the buffer the next
    call writes.  A case the Python trainer cannot express goes through the C entry points."""
    x, t = (c.x, c.t) if x is None else (x, t)
    if ic.needs_c(c.cfg):
        return ic.run_c(c.cfg, c.state, x, t)
    out = (trainer or new_trainer(c)).loss_and_grad(*device_inputs(x, t))
    return dict(out, grads={k: v.clone() for k, v in out["grads"].items()})


def stats_after_a_step(c):
    """{running statistic: device tensor} after one training step, and num_batches_tracked where the trainer keeps it"""
    if ic.needs_c(c.cfg):
        return ic.run_c(c.cfg, c.state, c.x, c.t)["stats"], None
    fresh = new_trainer(c)
    fresh.step(*device_inputs(c.x, c.t))
    return fresh.state_dict(), fresh


def share(value, floor):
    return value / (MARGIN * max(floor, ULP))


def compare(c, out):
    """gradients, loss terms and output rows of `out` against the case's float64 reference; prints the share of each
    bound that is used and returns the shares {"grad", "null", "terms", "out"} with the worst tensor's name"""
    what = f"{c.name} (seed {c.seed}, offset {c.offset}): {ic.describe(c.cfg, c.N, c.M)}"
    terms, grads, out64, _ = c.reference
    floor = ic.floor_of(c)
    got = {k: v.cpu().numpy() for k, v in out["grads"].items()}
    assert sorted(got) == sorted(grads) and all(got[k].shape == grads[k].shape for k in grads), what
    worst, where, null = tw.compare(got, grads, tw.null_tensors(grads))
    used = {"grad": share(worst, floor["grad"]), "where": where, "null": null / NULL_BOUND, "terms": 0.0}
    print(f"{what}\n  worst gradient element {worst:.2e} of its tensor's maximum ({where}), {used['grad']:.3f} of the bound "
          f"{MARGIN * max(floor['grad'], ULP):.2e}; null tensors {null:.2e} of their layer's weight gradient, "
          f"{used['null']:.3f} of {NULL_BOUND:.1e}")
    failed = []
    for k in tw.TERMS:
        err, bound = abs(out[k] - terms[k]), MARGIN * max(floor["terms"], ULP) * abs(terms[k]) + 1e-6
        used["terms"] = max(used["terms"], err / bound)
        print(f"  {k}: {out[k]:.8g} against {terms[k]:.8g}, {err / bound:.3f} of the bound")
        if not err <= bound:
            failed.append(k)
    rows = out["out"].cpu().numpy().astype(np.float64)
    assert rows.shape == out64.shape, what
    err = np.abs(rows - out64).max() / np.abs(out64).max()
    used["out"] = share(err, floor["out"])
    print(f"  output rows {err:.2e} of their maximum, {used['out']:.3f} of the bound {MARGIN * max(floor['out'], ULP):.2e}")
    assert not failed, f"{what}: loss terms {failed}"
    assert used["out"] <= 1.0, f"{what}: output rows {err:.2e} of their maximum"
    assert used["grad"] <= 1.0, f"{what}: {where}: {worst:.2e} of its maximum"
    assert used["null"] <= 1.0, f"{what}: null tensors {null:.2e}"
    return used


def compare_stats(c):
    """after one step(): the running statistics against the twin's, num_batches_tracked advanced"""
    stats64 = c.reference[3]
    if not stats64:
        return 0.0
    floor = ic.floor_of(c)
    sd, trainer = stats_after_a_step(c)
    worst = 0.0
    for k, ref in stats64.items():
        e = np.abs(sd[k].cpu().numpy() - ref).max() / np.abs(ref).max()
        worst = max(worst, share(e, floor["stats"]))
        assert e <= MARGIN * max(floor["stats"], ULP), (c.name, k, e)
        if trainer is not None:
            tracked = sd[k.rsplit(".", 1)[0] + ".num_batches_tracked"]
            assert int(tracked) == 4 and tracked.dtype == torch.int64, (c.name, k)     # (random_state starts at 3)
    print(f"  running statistics {worst:.3f} of the bound {MARGIN * max(floor['stats'], ULP):.2e}")
    return worst


def same_bits(a, b, what):
    for k in tw.TERMS:
        assert a[k] == b[k], f"{what}: {k}"
    assert torch.equal(a["out"], b["out"]), f"{what}: out"
    assert sorted(a["grads"]) == sorted(b["grads"])
    for k, g in a["grads"].items():
        assert torch.equal(g, b["grads"][k]), f"{what}: {k}"


@pytest.mark.parametrize("name", list(ic.EDGES))
def test_edge_matches_float64_twin(name):
    """Observed on MI355X, the largest share of each bound over the 13 edges: gradients 0.11 (one_layer_dense_flag,
    _backbone._linear_layers.0.weight: 9.3e-6 of its maximum against a floor of 8.2e-6), loss terms 0.08, output rows
    0.13, running statistics 0.08; null tensors at most 2.4e-6 of their layer's weight gradient."""
    c = ic.edge(name)
    assert ic.accepted(ic.tabled(c)), ic.tabled(c)
    compare(c, run(c))
    compare_stats(c)


@pytest.mark.parametrize("name", INFERENCE)
def test_inference_network_on_what_training_wrote(name):
    """``net()`` -- the inference kernels on the state one step() leaves -- on the first point set against the twin in
    eval() mode on that state, within the inference path's own bound (1e-4 of the row's maximum,
    test_init_network_gpu.py)"""
    c = ic.edge(name)
    fresh = new_trainer(c)
    fresh.step(*device_inputs(c.x, c.t))
    sd = fresh.state_dict()
    twin = tw.Twin(c.cfg, {k: v.cpu().numpy() for k, v in sd.items()})
    ref = np.concatenate([np.ravel(v) for v in twin.evaluate(c.x[:1])])
    with torch.no_grad():
        latent, position, scale, orientation = fresh.net()(torch.tensor(c.x[0], dtype=torch.float32, device="cuda")[None])
    row = torch.cat([latent[0], position[0], scale.reshape(1), orientation[0]]).cpu().numpy()
    err = np.abs(row - ref).max() / np.abs(ref).max()
    print(f"{name}: the inference network's row {err:.2e} of its maximum, bound 1e-4")
    assert row.shape == ref.shape and err <= 1e-4


@pytest.mark.parametrize("name", ["rows_1025", "dense_residual_70_70_140"])
def test_same_inputs_same_bits(name):
    """the fixed-order records: two weight-gradient records (1 024 rows + 1), and per-sample records of a second column
    block, give the same bits twice -- terms, output rows, every gradient"""
    c = ic.edge(name)
    t = new_trainer(c)
    same_bits(run(c, t), run(c, t), name)
    same_bits(run(c, t), run(c), f"{name}, a fresh trainer")


@pytest.mark.parametrize("name, other", [("rows_1025", (2, 9)), ("dense_residual_70_70_140", (3, 130)),
                                         ("in_1_dense_residual_m3", (5, 40))])
def test_batch_shape_reuse(name, other):
    """one trainer at (N, M), at (N', M'), at (N, M) again: the third result is the first bit for bit and the middle
    one a fresh trainer's -- ``_buffers`` keeps one shape at a time, and the workspace layout moves with M"""
    c = ic.edge(name)
    assert other != (c.N, c.M)
    x2, t2 = ic.inputs(c.cfg, *other, c.seed + 50)
    t = new_trainer(c)
    first = run(c, t)
    middle = run(c, t, x2, t2)
    third = run(c, t)
    assert middle["out"].shape[0] == other[0] and list(t._batch) == [(c.N, c.M)]
    same_bits(third, first, f"{name}: back at {(c.N, c.M)}")
    same_bits(middle, run(c, None, x2, t2), f"{name}: at {other}")
