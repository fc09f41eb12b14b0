#!/usr/bin/env python3
"""Capture tests/golden/vae_train_mug.npz by IMPORTING the reference's SDFVAE (sdfest/vae/sdf_vae.py) with the trained
mug checkpoint (tests/initilization/vae_model/mug.{yaml,pt}) in float64; dev container only.

One training iteration's loss and parameter gradients, the loss written as sdfest/vae/scripts/train.py:208-229, :271-281:
  * input    blobs_sdf(0), blobs_sdf(1) (N = 2); eps = encoder_twin.normal_eps(5, 2, 8) in place of torch.randn
  * weights  l2_small 1, l2_large 0.5, l1_small 0.25, l1_large 0.125, kld 1 (every term live)
  * phases   "warm": no clamp, no mask, kld weight 0; "post": tsdf = 0.1 (prepare_input, the masked clamp, kld weight 1)
Stored per phase: the five terms and the total; per parameter tensor the gradient's max-abs, L2 norm and every 97th
element of the flattened gradient (float64).  No grid and no full gradient.

Usage:  python tools/make_vae_train_goldens.py [--ref /root/reference]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "vae_train_mug.npz")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sdfest_amd.synthetic import blobs_sdf  # noqa: E402  (input generator only)
from encoder_twin import normal_eps  # noqa: E402

SEED, TSDF, EVERY = 5, 0.1, 97
W = {"l2_small": 1.0, "l2_large": 0.5, "l1_small": 0.25, "l1_large": 0.125, "kld": 1.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    import torch
    import yaml
    sys.path.insert(0, a.ref)
    from sdfest.vae import sdf_vae
    with open(os.path.join(a.ref, "tests/initilization/vae_model/mug.yaml")) as f:
        cfg = yaml.safe_load(f)
    state = torch.load(os.path.join(a.ref, "tests/initilization/vae_model/mug.pt"), map_location="cpu")
    eps = torch.tensor(normal_eps(SEED, 2, cfg["latent_size"]), dtype=torch.float64)
    out = {"seed": np.int64(SEED), "tsdf": np.float64(TSDF), "every": np.int64(EVERY),
           "weights": np.array([W[k] for k in ("l2_small", "l2_large", "l1_small", "l1_large", "kld")])}
    for phase, tsdf, post in (("warm", False, False), ("post", TSDF, True)):
        vae = sdf_vae.SDFVAE(sdf_size=64, latent_size=cfg["latent_size"], encoder_dict=cfg["encoder"],
                             decoder_dict=cfg["decoder"], device="cpu", tsdf=tsdf)
        vae.load_state_dict(state)
        vae.double()
        x = torch.tensor(np.stack([blobs_sdf(0), blobs_sdf(1)])[:, None], dtype=torch.float64)
        if post:
            vae.prepare_input(x)
        means, log_var = vae.encoder(x)
        z = eps * torch.exp(0.5 * log_var) + means
        recon = vae.decoder(z, enforce_tsdf=False)
        if tsdf is not False and post:
            mask = torch.logical_and(torch.abs(x) >= tsdf, torch.abs(recon) >= tsdf)
            out[f"{phase}_mask_fraction"] = np.float64(mask.double().mean().item())
            temp = recon
            recon = temp.clone()
            recon[mask] = temp[mask].clamp(-tsdf, tsdf)
        l1_error = torch.abs(recon - x)
        l2_error = l1_error ** 2
        l2_small = torch.sum(l2_error[torch.abs(x) < 0.1])
        l2_large = torch.sum(l2_error[torch.abs(x) >= 0.1])
        l1_small = torch.sum(l1_error[torch.abs(x) < 0.1])
        l1_large = torch.sum(l1_error[torch.abs(x) >= 0.1])
        kld = -0.5 * torch.sum(1 + log_var - means.pow(2) - log_var.exp())
        loss = (W["l2_small"] * l2_small + W["l2_large"] * l2_large + W["l1_small"] * l1_small
                + W["l1_large"] * l1_large + kld * (W["kld"] if post else 0))
        loss.backward()
        out[f"{phase}_terms"] = np.array([t.item() for t in (l2_small, l2_large, l1_small, l1_large, kld, loss)])
        for name, p in vae.named_parameters():
            g = p.grad.detach().numpy().reshape(-1)
            out[f"{phase}/{name}/stats"] = np.array([np.abs(g).max(), np.sqrt((g * g).sum())])
            out[f"{phase}/{name}/samples"] = g[::EVERY].copy()
        print(f"  {phase}: terms {out[f'{phase}_terms']}")
    out["names"] = np.array([n for n, _ in vae.named_parameters()])
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; mask fraction {out['post_mask_fraction']:.3f}")


if __name__ == "__main__":
    main()
