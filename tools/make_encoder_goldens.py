#!/usr/bin/env python3
"""Capture tests/golden/encoder_mug.npz by IMPORTING the reference's SDFVAE (sdfest/vae/sdf_vae.py) with the trained
mug checkpoint (tests/initilization/vae_model/mug.pt); dev container only.

Stores the mug ENCODER's weights (the decoder's are in mug_decoder_weights.npz) and the reference's fp32 CPU
``means`` / ``log_var`` for inputs that the tests rebuild themselves -- no grid is stored:
  * z0      decoder_mug.npz:z0_full (the decoded first latent)
  * sphere  sdfest_amd.synthetic.sphere_sdf(0.5)
  * blobs   sdfest_amd.synthetic.blobs_sdf(seed) for BLOB_SEEDS
  * tsdf    blobs_sdf(0) through the reference's prepare_input with tsdf = TSDF (SDFEncoder of the same weights)

Usage:  python tools/make_encoder_goldens.py [--ref /root/reference]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "encoder_mug.npz")
sys.path.insert(0, ROOT)

from sdfest_amd.synthetic import blobs_sdf, sphere_sdf  # noqa: E402  (input generators only)

BLOB_SEEDS = (0, 1, 2, 3)
TSDF = 0.1


def inputs():
    z0 = np.load(os.path.join(ROOT, "tests", "golden", "decoder_mug.npz"))["z0_full"].astype(np.float32)
    grids = {"z0": z0, "sphere": sphere_sdf(0.5)}
    for s in BLOB_SEEDS:
        grids[f"blobs{s}"] = blobs_sdf(s)
    return grids


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
    vae = sdf_vae.SDFVAE(sdf_size=64, latent_size=cfg["latent_size"], encoder_dict=cfg["encoder"],
                         decoder_dict=cfg["decoder"], device="cpu")
    vae.load_state_dict(state)
    vae.eval()
    out = {k: v.numpy().astype(np.float32) for k, v in state.items() if k.startswith("encoder.")}
    print(f"  encoder tensors: {len(out)}, params: {sum(v.size for v in out.values())}")
    grids = inputs()
    names = list(grids)
    x = torch.tensor(np.stack([grids[n] for n in names])[:, None])
    with torch.no_grad():
        means, log_var = vae.encoder(x)
        tvae = sdf_vae.SDFVAE(sdf_size=64, latent_size=cfg["latent_size"], encoder_dict=cfg["encoder"],
                              decoder_dict=cfg["decoder"], device="cpu", tsdf=TSDF)
        tvae.load_state_dict(state)
        tvae.eval()
        xt = torch.tensor(blobs_sdf(0)[None, None])
        tvae.prepare_input(xt)
        tm, tl = tvae.encoder(xt)
    out["names"] = np.array(names)
    out["means"] = means.numpy()
    out["log_var"] = log_var.numpy()
    out["tsdf"] = np.float32(TSDF)
    out["tsdf_means"] = tm.numpy()
    out["tsdf_log_var"] = tl.numpy()
    out["latent_size"] = np.int32(cfg["latent_size"])
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; means[0] = {out['means'][0]}")


if __name__ == "__main__":
    main()
