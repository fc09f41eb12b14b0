"""CPU twin of sdfest_amd/csrc/initnet_train.hip: one training iteration of the initialisation network
(sdfest/initialization/scripts/train.py:130-150, _compute_loss :211-287; pointnet.py:62-96; sdf_pose_network.py:88-115) as
a plain torch statement -- the layers written out over tensors that require grad, autograd, torch.optim.Adam -- in float64
(or any dtype).  Never reads the reference and never routes through sdfest_amd; tests/test_init_train_cpu.py checks it
against tests/golden/init_train.npz, which tools/make_init_train_goldens.py captured from the reference's own modules.

Also here: the small configurations and the GPU tests' cases (``CASES``), their inputs, the two conditions on those
inputs (``branch_margin``, ``null_tensors``) and the "fp32 floor" -- how far torch fp32 on the CPU lies from float64 on
the same inputs -- by which the GPU tests' bounds are set.  ``python tests/init_train_twin.py`` rewrites the table of
floors, tests/golden/init_train_floors.json."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

TERMS = ("latent", "position", "scale", "orientation", "total")
WEIGHTS = {"latent_weight": 1.0, "position_weight": 1000.0, "scale_weight": 1000.0, "orientation_weight": 5.0}
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
FLOORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_train_floors.json")

MUG = {"backbone": {"in_size": 3, "mlp_out_sizes": [128, 128, 128, 128, 1024], "batchnorm": True, "dense": True,
                    "residual": True},
       "head": {"in_size": 1024, "mlp_out_sizes": [512, 256, 128], "batchnorm": True},
       "orientation_repr": "discretized", "orientation_grid_resolution": 1, "cells": 576, "latent_size": 8}
# dense + residual + BatchNorm; the last width is NOT twice the one before (that ties the final pooling by construction)
P16 = {"backbone": {"in_size": 3, "mlp_out_sizes": [16, 16, 16, 40], "batchnorm": True, "dense": True, "residual": True},
       "head": {"in_size": 40, "mlp_out_sizes": [24, 16], "batchnorm": True},
       "orientation_repr": "discretized", "orientation_grid_resolution": 0, "cells": 72, "latent_size": 3}
B16 = {"backbone": {"in_size": 3, "mlp_out_sizes": [16, 24, 32], "batchnorm": True, "dense": False, "residual": False},
       "head": {"in_size": 32, "mlp_out_sizes": [24, 16], "batchnorm": True},
       "orientation_repr": "discretized", "orientation_grid_resolution": 0, "cells": 72, "latent_size": 3}
Q16 = {"backbone": {"in_size": 3, "mlp_out_sizes": [16, 16, 40], "batchnorm": False, "dense": False, "residual": True},
       "head": {"in_size": 40, "mlp_out_sizes": [24], "batchnorm": False},
       "orientation_repr": "quaternion", "cells": 0, "latent_size": 2}
# a residual link INTO THE LAST backbone layer: the set maximum is taken over prev_out + relu and its gradient also goes,
# ungated, to prev_out at the maximum's row.  R32: dense + residual with a last layer as wide as [F | G] together (its
# broadcast half ties by construction where the ReLU is zero for every row); R16: residual alone, three equal widths.
R32 = {"backbone": {"in_size": 3, "mlp_out_sizes": [16, 16, 32], "batchnorm": True, "dense": True, "residual": True},
       "head": {"in_size": 32, "mlp_out_sizes": [24, 16], "batchnorm": True},
       "orientation_repr": "discretized", "orientation_grid_resolution": 0, "cells": 72, "latent_size": 3}
R16 = {"backbone": {"in_size": 3, "mlp_out_sizes": [16, 16, 16], "batchnorm": False, "dense": False, "residual": True},
       "head": {"in_size": 16, "mlp_out_sizes": [24], "batchnorm": False},
       "orientation_repr": "quaternion", "cells": 0, "latent_size": 2}
CONFIGS = {"P16": P16, "B16": B16, "Q16": Q16, "mug": MUG, "R32": R32, "R16": R16}
# (config, N, M, seed): M = 37 below one 64-row tile, M = 130 crosses a tile inside a set, 5 x 300 rows = several row
# blocks and two weight-gradient records; every BatchNorm case has N >= 4.  The seeds are the first for which
# branch_margin() >= 1e-5 and the fp32 floor of the gradients is <= 1e-4 (test_init_train_cpu.py asserts both).
# The cases with an offset (1 500 rows, the mug widths) have channels whose ReLU is almost entirely on or off: the mixed
# ReLU masks inside a channel, and the BatchNorm backward over them, are covered by the M = 37 and M = 130 cases.
CASES = [("P16", 4, 37, 0, 0.0), ("P16", 4, 130, 1, 0.0), ("P16", 5, 300, 1, 2.0), ("B16", 4, 37, 1, 0.0),
         ("B16", 5, 300, 0, 2.0), ("Q16", 2, 37, 0, 0.0), ("Q16", 3, 130, 0, 0.0), ("Q16", 5, 300, 0, 0.0),
         ("mug", 4, 64, 26, 3.0), ("R32", 4, 130, 1, 0.0), ("R16", 3, 130, 0, 0.0)]   # (last: random_state's offset)
TRAJECTORY = ("P16", 6, 37, 0, 20)     # config, N, M, seed, steps


def train_config(cfg, **more):
    """the trainer's config of a small configuration: the reference's keys"""
    out = {"backbone_type": "VanillaPointNet", "head_type": "SDFPoseHead", "backbone": dict(cfg["backbone"]),
           "head": dict(cfg["head"]), "orientation_repr": cfg["orientation_repr"],
           "vae": {"latent_size": cfg["latent_size"]}, "learning_rate": 1e-3, "batch_size": 4, "iterations": 10}
    if "orientation_grid_resolution" in cfg:
        out["orientation_grid_resolution"] = cfg["orientation_grid_resolution"]
    out.update(WEIGHTS)
    out.update(more)
    return out


def n_out(cfg):
    return cfg["latent_size"] + 4 + (cfg["cells"] if cfg["cells"] else 4)


def parameter_shapes(cfg):
    """[(key, shape)] in the reference's parameters() order"""
    bb, hd = cfg["backbone"], cfg["head"]
    out, width = [], bb["in_size"]
    for i, c in enumerate(bb["mlp_out_sizes"]):
        out += [(f"_backbone._linear_layers.{i}.weight", (c, width)), (f"_backbone._linear_layers.{i}.bias", (c,))]
        width = 2 * c if bb.get("dense") else c
    if bb["batchnorm"]:
        for i, c in enumerate(bb["mlp_out_sizes"]):
            out += [(f"_backbone._bn_layers.{i}.weight", (c,)), (f"_backbone._bn_layers.{i}.bias", (c,))]
    width = hd["in_size"]
    for i, c in enumerate(hd["mlp_out_sizes"]):
        out += [(f"_head._linear_layers.{i}.weight", (c, width)), (f"_head._linear_layers.{i}.bias", (c,))]
        width = c
    if hd["batchnorm"]:
        for i, c in enumerate(hd["mlp_out_sizes"]):
            out += [(f"_head._bn_layers.{i}.weight", (c,)), (f"_head._bn_layers.{i}.bias", (c,))]
    out += [("_head._final_layer.weight", (n_out(cfg), width)), ("_head._final_layer.bias", (n_out(cfg),))]
    return out


def stat_shapes(cfg):
    """[(BatchNorm prefix, channels)] in the statistics buffer's order"""
    out = []
    for part in ("backbone", "head"):
        if cfg[part]["batchnorm"]:
            out += [(f"_{part}._bn_layers.{i}", c) for i, c in enumerate(cfg[part]["mlp_out_sizes"])]
    return out


def random_state(cfg, seed, offset=0.0):
    """float64 numpy state dict: torch's default Linear initialisation, BatchNorm affine parameters away from (1, 0) and
    running statistics away from (0, 1), so that a kernel that ignores any of them cannot pass.  `offset` > 0 moves
    every backbone BatchNorm bias by +-offset x its weight (the sign drawn per channel): a channel's ReLU then cuts at +-offset
    standard deviations instead of near the mean, where the rows are dense -- with tens of thousands of rows x channels
    some pre-activation always lies within 1e-5 of zero otherwise, and branch_margin() cannot hold."""
    rng = np.random.default_rng(1000 + seed)
    state, bound = {}, 0.0
    for key, shape in parameter_shapes(cfg):
        if "_bn_layers" in key:
            if key.endswith("weight"):
                state[key] = rng.uniform(0.5, 1.5, shape)
            else:
                gamma = state[key[:-len("bias")] + "weight"]
                shift = offset if key.startswith("_backbone") else 0.0      # (the head's N rows are few)
                state[key] = 0.2 * rng.standard_normal(shape) + shift * gamma * rng.choice([-1.0, 1.0], shape)
        else:
            if len(shape) > 1:
                bound = 1.0 / np.sqrt(shape[1])
            state[key] = rng.uniform(-bound, bound, shape)
    for prefix, c in stat_shapes(cfg):
        state[prefix + ".running_mean"] = 0.1 * rng.standard_normal(c)
        state[prefix + ".running_var"] = rng.uniform(0.5, 1.5, c)
        state[prefix + ".num_batches_tracked"] = np.array(3, dtype=np.int64)
    return {k: (v if v.dtype == np.int64 else np.asarray(v, np.float32).astype(np.float64)) for k, v in state.items()}


def inputs(cfg, N, M, seed):
    """(points (N, M, in_size), targets) as float32-representable float64 numpy arrays: centred point sets the size of
    an object 10 cm across"""
    rng = np.random.default_rng(100 + seed)
    d = cfg["backbone"]["in_size"]
    x = rng.normal(size=(N, M, d)) * np.resize(np.array([0.05, 0.04, 0.03]), d)
    x = x - x.mean(1, keepdims=True)
    L, C = cfg["latent_size"], cfg["cells"]
    q = rng.normal(size=(N, 4))
    t = {"latent_shape": rng.normal(size=(N, L)), "position": rng.normal(size=(N, 3)) * 0.01,
         "scale": rng.uniform(0.05, 0.15, N)}
    t["orientation"] = rng.integers(0, C, N).astype(np.int64) if C else q / np.linalg.norm(q, axis=1, keepdims=True)
    f32 = lambda a: a if a.dtype == np.int64 else a.astype(np.float32).astype(np.float64)
    return f32(x), {k: f32(v) for k, v in t.items()}


def _batchnorm(u, p, prefix, training, stats):
    """BatchNorm1d over the rows of u (R, C); returns (y, {new running statistics})"""
    g, b = p[prefix + ".weight"], p[prefix + ".bias"]
    if not training:
        return (u - stats[prefix + ".running_mean"]) / torch.sqrt(stats[prefix + ".running_var"] + BN_EPS) * g + b, {}
    mean, var = u.mean(0), u.var(0, unbiased=False)
    new = {}
    if stats is not None:
        R = u.shape[0]
        new[prefix + ".running_mean"] = ((1 - BN_MOMENTUM) * stats[prefix + ".running_mean"] + BN_MOMENTUM * mean).detach()
        new[prefix + ".running_var"] = ((1 - BN_MOMENTUM) * stats[prefix + ".running_var"]
                                       + BN_MOMENTUM * var * R / (R - 1)).detach()
    return (u - mean) / torch.sqrt(var + BN_EPS) * g + b, new


def forward(p, cfg, x, training=True, stats=None, trace=None):
    """the head's output rows (N, L + 4 + C) or (N, L + 8) -- the quaternion BEFORE its normalisation -- and the updated
    running statistics.  `trace` (a dict) receives what branch_margin() looks at."""
    bb, hd = cfg["backbone"], cfg["head"]
    N, S = x.shape[0], x.shape[1]
    out = prev = x
    new_stats, pre, pools = {}, [], []
    n = len(bb["mlp_out_sizes"])
    for i, c in enumerate(bb["mlp_out_sizes"]):
        out = F.linear(out, p[f"_backbone._linear_layers.{i}.weight"], p[f"_backbone._linear_layers.{i}.bias"])
        if bb["batchnorm"]:
            y, st = _batchnorm(out.reshape(-1, c), p, f"_backbone._bn_layers.{i}", training, stats)
            new_stats.update(st)
            out = y.reshape(N, S, c)
        pre.append(out)
        out = torch.relu(out)
        if bb.get("dense"):
            out_max = torch.max(out, 1, keepdim=True)[0]
            if i != n - 1:
                pools.append(out)
                out = torch.cat((out, out_max.expand(-1, S, -1)), dim=2)
        if bb.get("residual") and prev.shape == out.shape:
            out = prev + out
        prev = out
    pools.append(out)
    out = torch.max(out, 1)[0]
    for i, c in enumerate(hd["mlp_out_sizes"]):
        out = F.linear(out, p[f"_head._linear_layers.{i}.weight"], p[f"_head._linear_layers.{i}.bias"])
        if hd["batchnorm"]:
            out, st = _batchnorm(out, p, f"_head._bn_layers.{i}", training, stats)
            new_stats.update(st)
        pre.append(out)
        out = torch.relu(out)
    out = F.linear(out, p["_head._final_layer.weight"], p["_head._final_layer.bias"])
    if trace is not None:
        trace["pre"], trace["pools"] = pre, pools
    return out, new_stats


def split(out, cfg):
    """(latent, position, scale, orientation): the quaternion normalised (sdf_pose_network.py:97-101)"""
    L = cfg["latent_size"]
    o = out[:, L + 4:]
    if not cfg["cells"]:
        o = o / torch.sqrt(torch.sum(o ** 2, 1, keepdim=True))
    return out[:, :L], out[:, L:L + 3], out[:, L + 3], o


def loss(out, targets, cfg, weights=WEIGHTS):
    """the five numbers of _compute_loss as a dict of tensors"""
    latent, position, scale, orientation = split(out, cfg)
    t = {"latent": F.mse_loss(latent, targets["latent_shape"]), "position": F.mse_loss(position, targets["position"]),
         "scale": F.mse_loss(scale, targets["scale"])}
    if cfg["cells"]:
        t["orientation"] = F.cross_entropy(orientation, targets["orientation"])
    else:   # quaternion_utils.simple_quaternion_loss
        t["orientation"] = torch.mean(1 - torch.sum(orientation * targets["orientation"], 1) ** 2)
    t["total"] = sum(weights[k + "_weight"] * t[k] for k in TERMS[:4])
    return t


class Twin:
    def __init__(self, cfg, state, dtype=torch.float64, lr=1e-3, weights=WEIGHTS):
        self.cfg, self.dtype, self.weights = cfg, dtype, weights
        self.p = {k: torch.tensor(np.asarray(state[k]), dtype=dtype, requires_grad=True) for k, _ in parameter_shapes(cfg)}
        self.stats = {f"{pre}.{s}": torch.tensor(np.asarray(state[f"{pre}.{s}"]), dtype=dtype)
                      for pre, _ in stat_shapes(cfg) for s in ("running_mean", "running_var")}
        self.opt = torch.optim.Adam(list(self.p.values()), lr=lr)

    def _tensors(self, x, targets):
        t = {k: torch.tensor(v) if v.dtype == np.int64 else torch.tensor(v, dtype=self.dtype) for k, v in targets.items()}
        return torch.tensor(x, dtype=self.dtype), t

    def loss_and_grad(self, x, targets, trace=None):
        """(terms: floats, grads: numpy, out rows, the running statistics one step on); nothing is updated"""
        x, t = self._tensors(x, targets)
        for v in self.p.values():
            v.grad = None
        out, new_stats = forward(self.p, self.cfg, x, True, self.stats, trace)
        terms = loss(out, t, self.cfg, self.weights)
        terms["total"].backward()
        return ({k: float(v.detach()) for k, v in terms.items()}, {k: v.grad.numpy().astype(np.float64) for k, v in self.p.items()},
                out.detach().numpy().astype(np.float64), {k: v.numpy().astype(np.float64) for k, v in new_stats.items()})

    def step(self, x, targets):
        x, t = self._tensors(x, targets)
        self.opt.zero_grad()
        out, new_stats = forward(self.p, self.cfg, x, True, self.stats)
        terms = loss(out, t, self.cfg, self.weights)
        terms["total"].backward()
        self.opt.step()
        self.stats.update(new_stats)
        return {k: float(v.detach()) for k, v in terms.items()}

    def evaluate(self, x):
        """eval() mode on (N, M, in_size): the split outputs as numpy"""
        with torch.no_grad():
            out, _ = forward(self.p, self.cfg, torch.tensor(x, dtype=self.dtype), False, self.stats)
            return [v.numpy().astype(np.float64) for v in split(out, self.cfg)]


def branch_margin(cfg, state, x, targets):
    """the smaller of: the smallest gap between the two largest entries of any pooled column with a positive maximum,
    relative to the largest pooled value of that pooling; the smallest |pre-activation| relative to its layer's largest.
    Columns that tie by construction (identical for every row, or zero for every row) are left out: the first row takes
    their gradient and no parameter gradient depends on the choice."""
    trace = {}
    with torch.no_grad():
        tw = Twin(cfg, state)
        forward(tw.p, cfg, torch.tensor(x), True, tw.stats, trace)
    worst = np.inf
    for pool in trace["pools"]:
        if pool.shape[1] < 2:
            continue
        top = torch.topk(pool, 2, dim=1).values
        live = (top[:, 0] > 0) & (pool.max(1)[0] > pool.min(1)[0])
        if live.any():
            worst = min(worst, float(((top[:, 0] - top[:, 1]) / top[:, 0].abs().max())[live].min()))
    for pre in trace["pre"]:
        worst = min(worst, float(pre.abs().min() / pre.abs().max()))
    return worst


def null_tensors(grads):
    """the tensors whose gradient is mathematically zero (what a following batch normalisation removes): float64 leaves
    ~1e-25 there; named by a maximum below 1e-9 of the largest gradient maximum"""
    top = max(np.abs(g).max() for g in grads.values())
    return sorted(k for k, g in grads.items() if np.abs(g).max() < 1e-9 * top)


def null_scale(name, grads):
    """what a null tensor's values are measured against: the float64 maximum of the same layer's weight gradient"""
    return np.abs(grads[name.rsplit(".", 1)[0] + ".weight"]).max()


def compare(got, ref, nulls):
    """(worst live element relative to its tensor's maximum and its name, worst null element relative to null_scale)"""
    worst, where, null = 0.0, None, 0.0
    for k, g64 in ref.items():
        err = np.abs(np.asarray(got[k], np.float64) - g64).max()
        if k in nulls:
            null = max(null, err / null_scale(k, ref))
        elif err / np.abs(g64).max() > worst:
            worst, where = err / np.abs(g64).max(), k
    return worst, where, null


def case_setup(case):
    """(config, state, points, targets) of a case"""
    name, N, M, seed, offset = case
    cfg = CONFIGS[name]
    return (cfg, random_state(cfg, seed, offset)) + inputs(cfg, N, M, seed)


def fp32_floor(case):
    """torch fp32 on the CPU against float64 on the case's own inputs: gradients (worst live element of its tensor's
    maximum), null tensors, loss terms (relative), output rows and running statistics (of the array's maximum)"""
    cfg, state, x, t = case_setup(case)
    t64, g64, o64, s64 = Twin(cfg, state).loss_and_grad(x, t)
    t32, g32, o32, s32 = Twin(cfg, state, torch.float32).loss_and_grad(x, t)
    worst, _, null = compare(g32, g64, null_tensors(g64))
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    return {"grad": worst, "null": null, "terms": max(abs(t32[k] - t64[k]) / abs(t64[k]) for k in TERMS),
            "out": rel(o32, o64), "stats": max([rel(s32[k], s64[k]) for k in s64] + [0.0])}


def trajectory_batch(it):
    """the fixed batch of step `it` of the trajectory test"""
    name, N, M, seed, _ = TRAJECTORY
    return inputs(CONFIGS[name], N, M, seed + 10 * it)


def trajectory_floor():
    """the worst per-step relative difference of the total loss, torch fp32 against float64, over the trajectory test"""
    name, N, M, seed, steps = TRAJECTORY
    cfg, state = CONFIGS[name], random_state(CONFIGS[name], seed)
    a, b = Twin(cfg, state), Twin(cfg, state, torch.float32)
    worst = 0.0
    for it in range(steps):
        x, t = trajectory_batch(it)
        ra, rb = a.step(x, t)["total"], b.step(x, t)["total"]
        worst = max(worst, abs(rb - ra) / abs(ra))
    return worst


def case_key(case):
    return "{}-N{}-M{}-s{}".format(*case[:4])


def compute_floors():
    torch.set_num_threads(1)     # one summation order wherever the table is made
    table = {case_key(c): fp32_floor(c) for c in CASES}
    table["trajectory"] = {"total": trajectory_floor()}
    return table


def load_floors():
    with open(FLOORS) as fh:
        return json.load(fh)


if __name__ == "__main__":
    floors = compute_floors()
    with open(FLOORS, "w") as fh:
        json.dump(floors, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for k, v in floors.items():
        print(k, {n: f"{e:.2e}" for n, e in v.items()})
