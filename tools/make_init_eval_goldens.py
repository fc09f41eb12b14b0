#!/usr/bin/env python3
"""Capture tests/golden/init_eval.npz: the initialisation network under eval() on a batch and the reference trainer's
four validation sums, from the reference's own modules in float64 on the CPU.

Backbone: the IMPORTED ``sdfest/initialization/pointnet.py::VanillaPointNet`` under ``.eval()``, with running
statistics away from (0, 1) (tests/init_train_twin.py::random_state).  Head: ``sdf_pose_network.py`` imports healpy
(absent), so ``SDFPoseHead.forward`` (:88-115) is restated from the torch modules it is made of, as
tools/make_init_train_goldens.py does.  Validation sums: ``scripts/train.py`` imports wandb, so
``_compute_validation_metrics`` (:439-481) and ``_mean_geodesic_distance`` (:344-363) are restated by reading, with the
IMPORTED ``quaternion_utils.geodesic_distance``.  The cells' quaternions are this project's ``SO3Grid`` (the reference's
needs healpy); the table used is stored.  Weights and inputs are tests/init_eval_twin.py's (seeded); per case and batch
the file holds the points, the set features, the output rows and the four sums.

Usage:  python tools/make_init_eval_goldens.py --reference /path/to/sdfest-repository
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")


def capture(case, which, table, pointnet, quaternion_utils):
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    import init_eval_twin as ev
    import init_train_twin as tw
    cfg, state, x, t, _, _ = ev.batch(case, which, table)
    bb, hd, L = cfg["backbone"], cfg["head"], cfg["latent_size"]
    T = lambda a: torch.tensor(a, dtype=torch.float64)
    net = pointnet.VanillaPointNet(bb["in_size"], bb["mlp_out_sizes"], bb["batchnorm"], residual=bb["residual"],
                                   dense=bb["dense"]).double()
    net.load_state_dict({k[len("_backbone."):]: torch.tensor(v) for k, v in state.items() if k.startswith("_backbone.")})
    hs = hd["mlp_out_sizes"]
    head = nn.ModuleDict({
        "_linear_layers": nn.ModuleList([nn.Linear(hd["in_size"] if i == 0 else hs[i - 1], c) for i, c in enumerate(hs)]),
        "_bn_layers": nn.ModuleList([nn.BatchNorm1d(c) for c in hs] if hd["batchnorm"] else []),
        "_final_layer": nn.Linear(hs[-1], tw.n_out(cfg))}).double()
    head.load_state_dict({k[len("_head."):]: torch.tensor(v) for k, v in state.items() if k.startswith("_head.")})
    net.eval()
    head.eval()
    with torch.no_grad():
        features = out = net(T(x))
        for i, layer in enumerate(head["_linear_layers"]):          # sdf_pose_network.py:88-93
            out = layer(out)
            if hd["batchnorm"]:
                out = head["_bn_layers"][i](out)
            out = F.relu(out)
        out = head["_final_layer"](out)
        position, scale, orientation = out[:, L:L + 3], out[:, L + 3], out[:, L + 4:]
        if cfg["orientation_repr"] == "quaternion":                 # :97-101
            orientation = orientation / torch.sqrt(torch.sum(orientation ** 2, 1, keepdim=True))
            predicted = orientation
        else:                                                       # train.py:348-353
            predicted = torch.empty((x.shape[0], 4), dtype=torch.float64)
            for i, v in enumerate(orientation):
                predicted[i, :] = torch.tensor(table[v.argmax().item()])
        sums = [torch.sum(torch.linalg.norm(position - T(t["position"]), dim=1)).item(),       # train.py:456-477
                torch.sum(torch.abs(scale - T(t["scale"]))).item(),
                torch.mean(quaternion_utils.geodesic_distance(T(t["quaternion"]), predicted)).item() * x.shape[0], 0.0]
        if cfg["orientation_repr"] == "discretized":
            sums[3] = F.cross_entropy(orientation, torch.tensor(t["orientation"]), reduction="sum").item()
    print(f"  {ev.case_key(case)} batch {which}: N = {x.shape[0]}, sums {sums}")
    return {"points": x, "features": features.numpy(), "out": out.numpy(), "sums": np.array(sums)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="root of the reference's repository (holds sdfest/)")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from sdfest.initialization import pointnet, quaternion_utils
    import init_eval_twin as ev
    import init_train_twin as tw
    tables = ev.grid_tables()
    out = {}
    for name, table in tables.items():
        if table is not None:
            out[f"grid_quats/{tw.CONFIGS[name]['orientation_grid_resolution']}"] = table
    for case in ev.CASES:
        for which in (0, 1):
            for k, v in capture(case, which, tables[case[0]], pointnet, quaternion_utils).items():
                out[f"{ev.case_key(case)}/{which}/{k}"] = v
    path = os.path.join(OUT, "init_eval.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
