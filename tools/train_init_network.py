#!/usr/bin/env python3
"""Train the single-shot initialisation network on the GPU: the reference's
``sdfest/initialization/scripts/train.py`` without wandb and visualisations.

Reads a YAML config with the reference's keys (``initialization/configs/default.yaml`` and what it includes, resolved
into one file): backbone_type, backbone, head_type, head, orientation_repr, orientation_grid_resolution, learning_rate,
batch_size, iterations, the four loss weights, ``vae`` (latent_size, encoder, decoder, tsdf and ``model``: the trained
VAE's state dict, optional sdf_size) and ``datasets``: {name: {type: SDFVAEViewDataset, probability, config_dict: the
generated-dataset block}}.  The samples are rendered on the GPU from the VAE's decoder (``SDFVAEViewGenerator``).  Writes
``{out}.pt`` (``torch.save`` of the state dict, the reference's ``SDFPoseNet`` keys) and ``{out}.yaml`` (the config and
``model: ./{name}.pt``, as train.py:178-184), which ``SDFPipeline`` loads as its ``init`` model; ``{out}.ckpt`` holds the
trainer's checkpoint for ``--checkpoint``.

Validation (train.py:439-481): with ``validation_iteration`` and ``validation_datasets``: {name: {type: SDFVAEViewDataset,
config_dict}} in the config, a fixed set per name is drawn once (``size`` samples where the block says so, otherwise
``--validation_samples``), the network runs over it under eval() every ``validation_iteration`` iterations, and the
reference's numbers are printed and written to ``{out}.validation.json`` as {iteration: {key: value}}.

Usage:  python tools/train_init_network.py --config cfg.yaml --out models/mug_init [--iterations N]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def dataset_block(config):
    """the one generated dataset of the config; raises for another type that is in use"""
    block = None
    for name, entry in (config.get("datasets") or {}).items():
        if float(entry.get("probability", 1.0)) == 0.0:
            continue
        if entry.get("type") != "SDFVAEViewDataset":
            raise NotImplementedError(f"datasets.{name}: type {entry.get('type')!r} is not implemented "
                                      "(only SDFVAEViewDataset)")
        if block is not None:
            raise NotImplementedError(f"datasets.{name}: mixing several datasets is not implemented")
        block = dict(entry.get("config_dict") or {})
    if block is None:
        raise KeyError("datasets: no SDFVAEViewDataset with a probability > 0")
    return block


def validation_blocks(config):
    """{name: generated-dataset block} of the config's validation sets (train.py:314-327); {} without
    ``validation_iteration`` or sets; raises for another dataset type"""
    if not config.get("validation_iteration"):
        return {}
    blocks = {}
    for name, entry in (config.get("validation_datasets") or {}).items():
        if entry.get("type") != "SDFVAEViewDataset":
            raise NotImplementedError(f"validation_datasets.{name}: type {entry.get('type')!r} is not implemented "
                                      "(only SDFVAEViewDataset)")
        blocks[name] = dict(entry.get("config_dict") or {})
    return blocks


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="YAML with the reference's training, network, vae and dataset keys")
    ap.add_argument("--out", required=True, help="output path without extension")
    ap.add_argument("--checkpoint", help="a trainer checkpoint to resume from")
    ap.add_argument("--iterations", type=int)
    ap.add_argument("--batch_size", type=int)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log_every", type=int, default=100)
    ap.add_argument("--validation_samples", type=int, default=1024,
                    help="samples of a validation set whose block has no `size`")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)

    import torch
    import yaml
    from sdfest_amd.generated_views import SDFVAEViewGenerator
    from sdfest_amd.init_train import SDFPoseNetTrainer
    from sdfest_amd.vae import SDFVAE
    with open(a.config) as f:
        config = yaml.safe_load(f)
    for key in ("iterations", "batch_size"):
        if getattr(a, key) is not None:
            config[key] = getattr(a, key)
    block = dataset_block(config)
    validation = validation_blocks(config)
    trainer = SDFPoseNetTrainer(config, seed=a.seed, device=a.device)
    if a.checkpoint:
        trainer.load_checkpoint(a.checkpoint)
    vae_cfg = config["vae"]
    if not vae_cfg.get("model") or not os.path.isfile(vae_cfg["model"]):
        ap.error(f"vae.model {vae_cfg.get('model')!r} is not a file (weights are not downloaded)")
    vae = SDFVAE.from_config(vae_cfg, torch.load(vae_cfg["model"], map_location="cpu"), device=a.device,
                             sdf_size=int(vae_cfg.get("sdf_size", 64)))
    block["orientation_repr"] = config["orientation_repr"]                       # train.py:55-60
    if "orientation_grid_resolution" in config:
        block["orientation_grid_resolution"] = config["orientation_grid_resolution"]
    block["pointcloud"] = True
    views = SDFVAEViewGenerator(block, vae.decoder, batch_size=int(trainer.config["batch_size"]), device=a.device,
                                seed=a.seed, prefetch_draws=True)
    if not validation:
        trainer.fit(views, log_every=a.log_every)
    else:
        sets, history = {}, {}
        for i, (name, vblock) in enumerate(validation.items()):
            size = int(vblock.pop("size", a.validation_samples))
            vblock.update({k: block[k] for k in ("orientation_repr", "orientation_grid_resolution") if k in block})
            vblock["pointcloud"] = True
            source = SDFVAEViewGenerator(vblock, vae.decoder, batch_size=int(trainer.config["batch_size"]),
                                         device=a.device, seed=a.seed + 7919 * (i + 1))
            sets[name] = trainer.validation_set(source, size, seed=a.seed)

        def report(iteration, named):
            print(f"iteration {iteration}: " + ", ".join(f"{k} {v:.6g}" for k, v in named.items()), flush=True)
            numbers = {k: v for k, v in named.items() if " validation " in k}
            if numbers:
                history[str(iteration)] = numbers

        trainer.fit(views, log_every=a.log_every, callback=report, validation=sets,
                    validation_every=int(config["validation_iteration"]))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".validation.json", "w") as f:
            json.dump(history, f, indent=1)
            f.write("\n")
    torch.cuda.synchronize()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    name = os.path.basename(a.out)
    torch.save({k: v.cpu() for k, v in trainer.state_dict().items()}, a.out + ".pt")
    saved = dict(trainer.config)
    saved["model"] = os.path.join(".", name + ".pt")
    with open(a.out + ".yaml", "w") as f:
        yaml.safe_dump(saved, f, sort_keys=False)
    trainer.save_checkpoint(a.out + ".ckpt")
    print(f"wrote {a.out}.pt, {a.out}.yaml and {a.out}.ckpt after {trainer.iteration} iterations")


if __name__ == "__main__":
    main()
