#!/usr/bin/env python3
"""Capture tests/golden/init_train.npz: one training iteration of the initialisation network from the reference's own
modules, in float64 on the CPU.

Backbone: the IMPORTED ``sdfest/initialization/pointnet.py::VanillaPointNet`` under ``.train()``.  Head:
``sdf_pose_network.py`` imports healpy (absent), so ``SDFPoseHead.forward`` (:88-115) is restated from the torch modules
it is made of (``nn.Linear``, ``nn.BatchNorm1d``, relu), as tools/make_goldens.py::make_init_network does.  Loss:
``scripts/train.py`` imports wandb, so ``_compute_loss`` (:211-287) is restated by reading, with the IMPORTED
``quaternion_utils.simple_quaternion_loss``.  Weights and inputs are tests/init_train_twin.py's (seeded), so the file
holds results only: the loss terms, and per parameter the gradient's maximum, norm and every k-th element; the head's
output rows; the running statistics after the step.

Two cases: the mug architecture at N = 4, M = 64 and Q16 (a plain quaternion network without BatchNorm) at N = 3, M = 130.

Usage:  python tools/make_init_train_goldens.py --reference /path/to/sdfest-repository
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
GOLDEN_CASES = {"mug": ("mug", 4, 64, 26, 3.0), "plain": ("Q16", 3, 130, 0, 0.0)}
EVERY = 97      # every k-th element of a gradient is kept


def capture(case, pointnet, quaternion_utils):
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    import init_train_twin as tw
    cfg, state, x, t = tw.case_setup(case)
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
    net.train()
    head.train()
    out = net(T(x))
    for i, layer in enumerate(head["_linear_layers"]):          # sdf_pose_network.py:88-93
        out = layer(out)
        if hd["batchnorm"]:
            out = head["_bn_layers"][i](out)
        out = F.relu(out)
    out = head["_final_layer"](out)
    orientation = out[:, L + 4:]
    if cfg["orientation_repr"] == "quaternion":                 # :97-101
        orientation = orientation / torch.sqrt(torch.sum(orientation ** 2, 1, keepdim=True))
    terms = {"latent": F.mse_loss(out[:, :L], T(t["latent_shape"])),          # train.py:241-278
             "position": F.mse_loss(out[:, L:L + 3], T(t["position"])), "scale": F.mse_loss(out[:, L + 3], T(t["scale"]))}
    if cfg["orientation_repr"] == "quaternion":
        terms["orientation"] = quaternion_utils.simple_quaternion_loss(orientation, T(t["orientation"]))
    else:
        terms["orientation"] = F.cross_entropy(orientation, torch.tensor(t["orientation"]))
    total = sum(tw.WEIGHTS[k + "_weight"] * v for k, v in terms.items())
    total.backward()
    res = {"terms": np.array([float(terms[k]) for k in tw.TERMS[:4]] + [float(total)]), "out": out.detach().numpy()}
    named = [("_backbone." + k, p) for k, p in net.named_parameters()] + [("_head." + k, p) for k, p in head.named_parameters()]
    res["keys"] = np.array([k for k, _ in named])
    for k, p in named:
        g = p.grad.numpy().ravel()
        res["grad_max/" + k] = np.abs(g).max()
        res["grad_norm/" + k] = np.linalg.norm(g)
        res["grad_every/" + k] = g[::EVERY].copy()
    for prefix, mod in (("_backbone.", net), ("_head.", head)):
        for k, b in mod.named_buffers():
            if not k.endswith("num_batches_tracked"):
                res["stat/" + prefix + k] = b.numpy().copy()
    print(f"  {tw.case_key(case)}: terms {res['terms']}, {len(named)} tensors")
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="root of the reference's repository (holds sdfest/)")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from sdfest.initialization import pointnet, quaternion_utils
    out = {}
    for tag, case in GOLDEN_CASES.items():
        for k, v in capture(case, pointnet, quaternion_utils).items():
            out[f"{tag}/{k}"] = v
    path = os.path.join(OUT, "init_train.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
