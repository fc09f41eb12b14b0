"""CPU twin of what sdfest_amd/csrc/initnet_eval.hip adds to the initialisation network: the validation numbers of the
reference's trainer (sdfest/initialization/scripts/train.py:344-374, :439-481) as a plain torch statement in float64 (or
any dtype), on the output rows of tests/init_train_twin.py::forward under eval().  Never reads the reference and never
computes through sdfest_amd; tests/test_init_eval_cpu.py checks it against tests/golden/init_eval.npz, which
tools/make_init_eval_goldens.py captured from the reference's own modules.

Also here: the GPU tests' cases, their inputs, the two conditions on those inputs (the top two logits of a sample at
least 1e-3 apart, so that the argmax is the same in every precision; |q . q*| <= 0.999, because acos is ill-conditioned
at 1) and the "fp32 floor" -- how far torch fp32 on the CPU lies from float64 on the same inputs -- by which the GPU
tests' bounds are set.  ``python tests/init_eval_twin.py`` rewrites the table of floors,
tests/golden/init_eval_floors.json."""
import json
import os

import numpy as np
import torch

import init_train_twin as tw

FLOORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_eval_floors.json")
SUMS = ("position", "scale", "geodesic", "nll")
LOGIT_GAP, MAX_DOT = 1e-3, 0.999
# (config, M, seed, (N of the first batch, N of the second)): M = 1, 37 below one 64-row tile, 64 exactly one, 65 one and
# a row, 130 three tiles; the mug widths at M = 130: cin = 128 > kChunk = two k chunks, 16 column blocks of the last
# layer, the 16-byte staging.  The seeds are the first for which both conditions hold (asserted by batch()).
CASES = [("P16", 37, 0, (3, 1)), ("P16", 130, 0, (1, 3)), ("B16", 65, 0, (3, 1)), ("Q16", 64, 0, (3, 1)),
         ("Q16", 1, 0, (3, 1)), ("R32", 130, 0, (3, 1)), ("R16", 37, 0, (3, 1)), ("mug", 130, 0, (2, 1))]


TRAIN_CASES = [tw.CASES[0], tw.CASES[5]]      # P16 N = 4 and Q16 N = 2 at M = 37: a discretized and a quaternion head


def case_key(case):
    return "{}-M{}-s{}".format(*case[:3])


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def targets_with_quaternion(cfg, t, N, seed):
    """the targets of tw.inputs plus "quaternion" (N, 4): the orientation itself for a quaternion head, otherwise drawn"""
    t = dict(t)
    if cfg["cells"]:
        q = np.random.default_rng(500 + seed).normal(size=(N, 4))
        t["quaternion"] = f32(q / np.linalg.norm(q, axis=1, keepdims=True))
    else:
        t["quaternion"] = t["orientation"]
    return t


def points(cfg, N, M, seed):
    """(N, M, in_size) float32-representable: tw.inputs' centred sets; a set of ONE point is its own centroid, so M = 1
    keeps the draw"""
    x, _ = tw.inputs(cfg, N, M, seed)
    if M == 1:
        d = cfg["backbone"]["in_size"]
        x = f32(np.random.default_rng(300 + seed).normal(size=(N, 1, d)) * np.resize(np.array([0.05, 0.04, 0.03]), d))
    return x


def state(case):
    return tw.random_state(tw.CONFIGS[case[0]], case[2])


def forward(cfg, st, x, dtype=torch.float64):
    """(features (N, C_last), output rows) of the network under eval() as tensors of `dtype`"""
    p = {k: torch.tensor(np.asarray(st[k]), dtype=dtype) for k, _ in tw.parameter_shapes(cfg)}
    stats = {f"{pre}.{s}": torch.tensor(np.asarray(st[f"{pre}.{s}"]), dtype=dtype)
             for pre, _ in tw.stat_shapes(cfg) for s in ("running_mean", "running_var")}
    trace = {}
    with torch.no_grad():
        out, _ = tw.forward(p, cfg, torch.tensor(x, dtype=dtype), False, stats, trace)
    return trace["pools"][-1].max(1)[0], out


def predicted_quaternions(out, cfg, grid_quats):
    """train.py:344-359: the argmax cell's quaternion (torch.argmax: the first maximum) or the head's, normalised"""
    o = out[:, cfg["latent_size"] + 4:]
    if cfg["cells"]:
        return torch.as_tensor(grid_quats, dtype=out.dtype)[o.argmax(1)]
    return o / torch.sqrt(torch.sum(o ** 2, 1, keepdim=True))


def samples(out, cfg, t, grid_quats=None):
    """the per-sample values of train.py:456-477, {name: (N,) tensor} ("nll": zeros for a quaternion head)"""
    L, T = cfg["latent_size"], lambda a: torch.tensor(a, dtype=out.dtype)
    q = predicted_quaternions(out, cfg, grid_quats)
    dot = torch.clip(torch.abs(torch.sum(T(t["quaternion"]) * q, dim=1)), 0, 1)     # quaternion_utils.geodesic_distance
    res = {"position": torch.linalg.norm(out[:, L:L + 3] - T(t["position"]), dim=1),
           "scale": torch.abs(out[:, L + 3] - T(t["scale"])), "geodesic": 2 * torch.acos(dot),
           "nll": torch.zeros(out.shape[0], dtype=out.dtype)}
    if cfg["cells"]:
        res["nll"] = torch.nn.functional.cross_entropy(out[:, L + 4:], torch.tensor(t["orientation"]), reduction="none")
    return res


def sums(out, cfg, t, grid_quats=None):
    """the four sums of train.py:456-477 over one batch, as floats"""
    return {k: float(v.sum()) for k, v in samples(out, cfg, t, grid_quats).items()}


def conditions(out, cfg, t, grid_quats):
    """(smallest gap between the two largest logits of a sample, or inf; largest |q . q*|)"""
    gap = np.inf
    if cfg["cells"]:
        top = torch.topk(out[:, cfg["latent_size"] + 4:], 2, dim=1).values
        gap = float((top[:, 0] - top[:, 1]).min())
    q = predicted_quaternions(out, cfg, grid_quats)
    return gap, float(torch.abs(torch.sum(torch.tensor(t["quaternion"]) * q, dim=1)).max())


def batch(case, which, grid_quats=None):
    """(config, state, points, targets, float64 features, float64 rows) of batch 0 or 1 of a case; asserts the two
    conditions on what it generates"""
    name, M, seed, Ns = case
    cfg, N, s = tw.CONFIGS[name], Ns[which], seed + 50 * which
    st, x = state(case), points(cfg, N, M, s)
    t = targets_with_quaternion(cfg, tw.inputs(cfg, N, M, s)[1], N, s)
    feat, out = forward(cfg, st, x)
    gap, dot = conditions(out, cfg, t, grid_quats)
    assert gap >= LOGIT_GAP and dot <= MAX_DOT, (case_key(case), which, gap, dot)
    return cfg, st, x, t, feat, out


def means(per_batch, counts):
    total = float(sum(counts))
    return {k: sum(b[k] for b in per_batch) / total for k in SUMS}


def fp32_floor(case, grid_quats=None):
    """torch fp32 on the CPU against float64 on the case's two batches: features, output rows and the parts of the
    4-tuple (worst element of the array's maximum), and per validation number the worst SAMPLE's difference over the
    float64 mean of both batches.  (Per sample, not of the mean: a mean's error is at most its worst sample's, while
    the fp32 errors of four samples can cancel in their mean to a figure that says nothing about another summation
    order.)"""
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())
    floor = {"features": 0.0, "out": 0.0, "tuple": 0.0}
    s64, worst = [], {k: 0.0 for k in SUMS}
    for which in (0, 1):
        cfg, st, x, t, feat, out = batch(case, which, grid_quats)
        feat32, out32 = forward(cfg, st, x, torch.float32)
        floor["features"] = max(floor["features"], rel(feat32, feat))
        floor["out"] = max(floor["out"], rel(out32, out))
        for a, b in zip(tw.split(out32, cfg), tw.split(out, cfg)):
            floor["tuple"] = max(floor["tuple"], rel(a, b))
        v64, v32 = samples(out, cfg, t, grid_quats), samples(out32, cfg, t, grid_quats)
        s64.append({k: float(v.sum()) for k, v in v64.items()})
        for k in SUMS:
            worst[k] = max(worst[k], float((v32[k].double() - v64[k]).abs().max()))
    m64 = means(s64, case[3])
    for k in SUMS:
        if m64[k] != 0.0:
            floor[k] = worst[k] / abs(m64[k])
    return floor


def train_batch(case, grid_quats=None):
    """(config, state, points, targets with "quaternion", float64 output rows under train()) of a case of
    init_train_twin.CASES: what ``SDFPoseNetTrainer.geodesic_distance`` is held against; asserts the two conditions"""
    cfg, st, x, t = tw.case_setup(case)
    t = targets_with_quaternion(cfg, t, case[1], case[3])
    out = torch.tensor(tw.Twin(cfg, st).loss_and_grad(x, t)[2])
    gap, dot = conditions(out, cfg, t, grid_quats)
    assert gap >= LOGIT_GAP and dot <= MAX_DOT, (tw.case_key(case), gap, dot)
    return cfg, st, x, t, out


def train_floor(case, grid_quats=None):
    """the batch mean geodesic distance of the train-mode rows: the worst sample's fp32 difference over the mean"""
    cfg, st, x, t, out = train_batch(case, grid_quats)
    out32 = torch.tensor(tw.Twin(cfg, st, torch.float32).loss_and_grad(x, t)[2], dtype=torch.float32)
    g64, g32 = samples(out, cfg, t, grid_quats)["geodesic"], samples(out32, cfg, t, grid_quats)["geodesic"]
    return {"geodesic": float((g32.double() - g64).abs().max() / g64.mean())}


def compute_floors(tables):
    """`tables`: {config name: the (C, 4) table of cell quaternions, or None}"""
    torch.set_num_threads(1)     # one summation order wherever the table is made
    table = {case_key(c): fp32_floor(c, tables[c[0]]) for c in CASES}
    table.update({"train-" + tw.case_key(c): train_floor(c, tables[c[0]]) for c in TRAIN_CASES})
    return table


def load_floors():
    with open(FLOORS) as fh:
        return json.load(fh)


def grid_tables():
    """{config name: float32-representable (C, 4) table of the grid's cells}: the project's own SO3Grid (host code; the
    reference's needs healpy), which tests/test_init_eval_cpu.py holds against the table stored with the golden"""
    from sdfest_amd.so3grid import SO3Grid
    by_resolution, out = {}, {}
    for name, cfg in tw.CONFIGS.items():
        if not cfg["cells"]:
            out[name] = None
            continue
        r = cfg["orientation_grid_resolution"]
        if r not in by_resolution:
            g = SO3Grid(r)
            by_resolution[r] = f32(np.stack([np.asarray(g.index_to_quat(i), np.float64) for i in range(g.num_cells())]))
        out[name] = by_resolution[r]
    return out


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    floors = compute_floors(grid_tables())
    with open(FLOORS, "w") as fh:
        json.dump(floors, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for k, v in floors.items():
        print(k, {n: f"{e:.2e}" for n, e in v.items()})
