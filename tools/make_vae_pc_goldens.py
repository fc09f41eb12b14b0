#!/usr/bin/env python3
"""Capture tests/golden/vae_train_pc.npz by IMPORTING the reference's SDFVAE (sdfest/vae/sdf_vae.py) with the trained mug
checkpoint (tests/initilization/vae_model/mug.{yaml,pt}) and its point cloud loss (sdfest/estimation/losses.py: pc_loss,
which at scale 1 is train.py's own pc_loss) in float64; dev container only.

One training iteration with EVERY term live, the loss written as sdfest/vae/scripts/train.py:208-281:
  * input    blobs_sdf(0), blobs_sdf(1) (N = 2); eps = encoder_twin.normal_eps(5, 2, 8) in place of torch.randn
  * weights  l2_small 1, l2_large 0.5, l1_small 0.25, l1_large 0.125, kld 1, pc 1
  * phases   "warm": no clamp, no mask, kld weight 0; "post": tsdf = 0.1 (prepare_input, the masked clamp, kld weight 1)
  * pc term  orientations = vae_pc_twin.orientations(5, 2) in place of random.random(); position (0, 0, -5), scale 1;
             the depth images are THIS repository's float64 oracle render of the (clamped) targets at threshold 0.01 with
             a 160 x 120, f = 80 camera, rounded to float32 and stored sparse (the reference's renderer is a GPU
             extension that does not build here, and the render is an input of the term, not part of it); the lift
             restates pointset_utils.py:57-77 as tools/make_goldens.py does (pointset_utils does not import here)
Stored per phase: the six terms plus pc; per parameter tensor the gradient's max-abs, L2 norm and every 97th element of
the flattened gradient (float64); the orientations; the depth images' non-zero pixels.

Usage:  python tools/make_vae_pc_goldens.py [--ref /root/reference]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "vae_train_pc.npz")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sdfest_amd.synthetic import blobs_sdf  # noqa: E402  (input generator only)
from encoder_twin import normal_eps  # noqa: E402
import vae_pc_twin as pt  # noqa: E402  (the orientation draw and the margin check only)

SEED, TSDF, EVERY = 5, 0.1, 97
W = {"l2_small": 1.0, "l2_large": 0.5, "l1_small": 0.25, "l1_large": 0.125, "kld": 1.0, "pc": 1.0}
CAM_W, CAM_H, F, CX, CY = 160, 120, 80.0, 80.0, 60.0      # pixel centre 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    import torch
    import yaml
    import oracle
    sys.path.insert(0, a.ref)
    from sdfest.vae import sdf_vae
    from sdfest.estimation import losses
    with open(os.path.join(a.ref, "tests/initilization/vae_model/mug.yaml")) as f:
        cfg = yaml.safe_load(f)
    state = torch.load(os.path.join(a.ref, "tests/initilization/vae_model/mug.pt"), map_location="cpu")
    eps = torch.tensor(normal_eps(SEED, 2, cfg["latent_size"]), dtype=torch.float64)
    quats = pt.orientations(SEED, 2)
    p = torch.tensor(pt.POSITION, dtype=torch.float64)
    s = torch.tensor(pt.SCALE, dtype=torch.float64)

    def depth_to_pointcloud(depth):  # pointset_utils.py:57-77, "opengl", no mask
        cx0, cy0 = CX - 0.5, CY - 0.5                   # Camera.get_pinhole_camera_parameters(0.0)
        idx = torch.nonzero(depth, as_tuple=True)
        z = depth[idx]
        return torch.stack(((idx[1].double() - cx0) * z / F, -(idx[0].double() - cy0) * z / F, -z), 1)

    out = {"seed": np.int64(SEED), "tsdf": np.float64(TSDF), "every": np.int64(EVERY), "orientations": quats,
           "camera": np.array([CAM_W, CAM_H, F, F, CX, CY]),
           "weights": np.array([W[k] for k in ("l2_small", "l2_large", "l1_small", "l1_large", "kld", "pc")])}
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
            temp = recon
            recon = temp.clone()
            recon[mask] = temp[mask].clamp(-tsdf, tsdf)
        l1_error = torch.abs(recon - x)
        l2_error = l1_error ** 2
        l2_small = torch.sum(l2_error[torch.abs(x) < 0.1])
        l2_large = torch.sum(l2_error[torch.abs(x) >= 0.1])
        l1_small = torch.sum(l1_error[torch.abs(x) < 0.1])
        l1_large = torch.sum(l1_error[torch.abs(x) >= 0.1])
        loss_pc = 0
        depths = np.zeros((2, CAM_H, CAM_W), dtype=np.float32)
        for b in range(2):
            q = torch.tensor(quats[b], dtype=torch.float64)
            d64 = oracle.render_forward(x[b, 0].numpy(), pt.POSITION, quats[b].astype(np.float64), [1.0 / pt.SCALE],
                                        CAM_W, CAM_H, CX, CY, F, F, pt.THRESHOLD, dtype=np.float64)[0]
            depths[b] = d64.astype(np.float32)
            pointcloud = depth_to_pointcloud(torch.tensor(depths[b], dtype=torch.float64))
            # the comparisons need no exclusions: no point near the in-volume mask's edge
            o = pt.canonical(pointcloud, pt.POSITION, quats[b], pt.SCALE)
            assert float((o.abs() - 1.0).abs().min()) > pt.MARGIN
            loss_pc = loss_pc + torch.sum(losses.pc_loss(pointcloud, p, q, s, recon[b, 0]) ** 2)
        kld = -0.5 * torch.sum(1 + log_var - means.pow(2) - log_var.exp())
        loss = (W["l2_small"] * l2_small + W["l2_large"] * l2_large + W["l1_small"] * l1_small
                + W["l1_large"] * l1_large + W["pc"] * loss_pc + kld * (W["kld"] if post else 0))
        loss.backward()
        out[f"{phase}_terms"] = np.array([t.item() for t in (l2_small, l2_large, l1_small, l1_large, kld, loss, loss_pc)])
        idx, val = pt.sparse(depths)
        out[f"{phase}_depth_index"], out[f"{phase}_depth_value"] = idx.astype(np.int32), val
        for name, prm in vae.named_parameters():
            g = prm.grad.detach().numpy().reshape(-1)
            out[f"{phase}/{name}/stats"] = np.array([np.abs(g).max(), np.sqrt((g * g).sum())])
            out[f"{phase}/{name}/samples"] = g[::EVERY].copy()
        print(f"  {phase}: terms {out[f'{phase}_terms']}; {idx.size} depth pixels")
    out["names"] = np.array([n for n, _ in vae.named_parameters()])
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
