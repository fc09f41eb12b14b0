"""CPU: the float64 twin of the VAE training iteration (tests/vae_train_twin.py) against the reference's golden
(tests/golden/vae_train_mug.npz, tools/make_vae_train_goldens.py) and against the encoder's and decoder's twins; the
argument checks of the C ABI's group 10 (no HIP call is made); what the trainer rejects; the checkpoint file; the
command line's --help."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import encoder_twin as et
import vae_train_twin as tw
from helpers import GOLDEN, ROOT


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "vae_train_mug.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def mug():
    return tw.mug_setup()


@pytest.mark.parametrize("phase, iteration", [("warm", 0), ("post", 1001)])
def test_twin_reproduces_reference_golden(golden, mug, phase, iteration):
    """both are float64 torch: only the summation order can differ -- terms to 1e-9 relative, gradient samples and norms
    to 1e-9 of each tensor's max-abs"""
    config, state = mug
    twin = tw.Twin(config, state)
    x = tw.blobs_at(64, (0, 1))
    eps = et.normal_eps(int(golden["seed"]), 2, 8)
    terms, grads, _ = twin.run(x, eps, iteration)
    got = np.array([terms[k] for k in tw.TERMS])
    assert np.all(np.abs(got - golden[f"{phase}_terms"]) <= 1e-9 * np.abs(golden[f"{phase}_terms"])), (got, golden[f"{phase}_terms"])
    assert sorted(grads) == sorted(golden["names"].tolist())
    every = int(golden["every"])
    for name, g in grads.items():
        top, norm = golden[f"{phase}/{name}/stats"]
        flat = g.reshape(-1)
        assert top > 0, name
        assert abs(np.abs(flat).max() - top) <= 1e-9 * top, name
        assert abs(np.sqrt((flat * flat).sum()) - norm) <= 1e-9 * top * np.sqrt(flat.size), name
        assert np.max(np.abs(flat[::every] - golden[f"{phase}/{name}/samples"])) <= 1e-9 * top, name
    if phase == "post":
        assert 0.5 < float(golden["post_mask_fraction"]) < 0.9      # the masked clamp is exercised


def test_twin_forward_is_the_encoder_and_decoder_twins(mug):
    from test_decoder_gpu import torch_decoder
    for config, state, seeds in ((mug[0], mug[1], (2,)), (tw.T16, tw.random_state(tw.T16, 3), (0, 1, 2))):
        D = config["sdf_size"]
        x = tw.blobs_at(D, seeds)
        eps = et.normal_eps(7, len(seeds), config["latent_size"])
        twin = tw.Twin(config, state)
        with torch.no_grad():
            means, log_var, z, recon = tw.forward(twin.params, config, torch.tensor(x).double(), torch.tensor(eps).double())
        m64, lv64 = et.torch_encoder(state, config["encoder"]["layer_infos"], x)
        assert torch.equal(means, m64) and torch.equal(log_var, lv64)
        out = torch_decoder(state, config["decoder"]["fc_layers"], config["decoder"]["conv_layers"], D, z)
        assert torch.equal(recon, out)


def test_parameter_layout_matches_the_library():
    from sdfest_amd import _lib
    from sdfest_amd.train import parameter_shapes
    from sdfest_amd.vae import parse_encoder_layers
    L = _lib.lib()
    for config in (tw.T16, tw.T8, tw.mug_setup()[0]):
        h = create(L, config)
        shapes = parameter_shapes(config)
        assert L.sdfr_vae_trainer_param_count(h) == sum(int(np.prod(s)) for _, s in shapes)
        enc = sum(int(np.prod(s)) for k, s in shapes if k.startswith("encoder."))
        assert L.sdfr_vae_trainer_encoder_param_count(h) == enc
        assert [k for k, _ in shapes] == sorted([k for k, _ in shapes], key=lambda k: not k.startswith("encoder."))
        assert L.sdfr_vae_trainer_tape_bytes(h, 2) > 0 and L.sdfr_vae_trainer_workspace_bytes(h, 2) > 0
        L.sdfr_vae_trainer_destroy(h)
    assert parse_encoder_layers(16, tw.T16["encoder"]["layer_infos"])["features"] == 12


def create(L, config, expect=0, **change):
    from sdfest_amd import _lib
    from sdfest_amd.vae import parse_encoder_layers
    arr = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    conv, fc = config["decoder"]["conv_layers"], config["decoder"]["fc_layers"]
    ops = arr(change.get("ops", parse_encoder_layers(config["sdf_size"], config["encoder"]["layer_infos"])["ops"]))
    a = dict(latent=config["latent_size"], fc=arr([l["out"] for l in fc]), ins=arr([l["in_size"] for l in conv]),
             cin=arr([l["in_channels"] for l in conv]), cout=arr([l["out_channels"] for l in conv]),
             k=arr([l["kernel_size"] for l in conv]), relu=arr([int(l["relu"]) for l in conv]),
             volume=config["sdf_size"], tsdf=float(config["tsdf"] or 0.0))
    a.update({k: (arr(v) if isinstance(v, list) else v) for k, v in change.items() if k != "ops"})
    h = ctypes.c_void_p()
    rc = L.sdfr_vae_trainer_create(a["latent"], len(a["fc"]), P(a["fc"]), len(a["ins"]), P(a["ins"]), P(a["cin"]),
                                   P(a["cout"]), P(a["k"]), P(a["relu"]), a["volume"], a["tsdf"],
                                   ops.reshape(-1, _lib.ABI["SDFR_ENC_OP_INTS"]).shape[0], P(ops), 0, ctypes.byref(h))
    assert rc == expect, (rc, L.sdfr_last_error())
    return h


def test_entry_points_validate_their_arguments_without_gpu():
    """argument errors are reported before any HIP call: NULL handle or buffer, N < 1, a short tape / workspace, and at
    creation what the inference handles reject, with their messages"""
    from sdfest_amd import _lib
    L = _lib.lib()
    err = lambda: L.sdfr_last_error()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)   # a non-NULL pointer that is never dereferenced
    h = create(L, tw.T16)
    big = 1 << 40
    # forward
    assert L.sdfr_vae_trainer_forward(None, q, q, 2, 0, 0, q, q, q, q, q, big, None) == -2 and b"NULL trainer" in err()
    assert L.sdfr_vae_trainer_forward(h, q, q, 0, 0, 0, q, q, q, q, q, big, None) == -1 and b"N=0" in err()
    assert L.sdfr_vae_trainer_forward(h, q, q, 70000, 0, 0, q, q, q, q, q, big, None) == -1
    for i in (1, 2, 6, 7, 8, 9, 10):
        args = [h, q, q, 2, 0, 0, q, q, q, q, q, big, None]
        args[i] = None
        assert L.sdfr_vae_trainer_forward(*args) == -2 and b"NULL pointer" in err(), i
    assert L.sdfr_vae_trainer_forward(h, q, q, 2, 0, 0, q, q, q, q, q, 64, None) == -3 and b"tape 64 <" in err()
    # loss
    w = (1.0, 0.5, 0.25, 0.125, 1.0)
    assert L.sdfr_vae_trainer_loss(None, q, q, q, q, 2, *w, 1, q, q, q, q, q, big, None) == -2
    assert L.sdfr_vae_trainer_loss(h, q, q, q, q, -1, *w, 1, q, q, q, q, q, big, None) == -1 and b"N=-1" in err()
    for i in (1, 2, 3, 4, 12, 13, 14, 15):
        args = [h, q, q, q, q, 2, *w, 1, q, q, q, q, q, big, None]
        args[i] = None
        assert L.sdfr_vae_trainer_loss(*args) == -2 and b"NULL pointer" in err(), i
    assert L.sdfr_vae_trainer_loss(h, q, q, q, q, 2, *w, 1, q, q, q, q, None, big, None) == -2 and b"workspace" in err()
    assert L.sdfr_vae_trainer_loss(h, q, q, q, q, 2, *w, 1, q, q, q, q, q, 100, None) == -3 and b"workspace 100 <" in err()
    # backward
    assert L.sdfr_vae_trainer_backward(None, q, q, 2, 0, q, q, q, q, q, q, q, q, q, big, None) == -2
    assert L.sdfr_vae_trainer_backward(h, q, q, 0, 0, q, q, q, q, q, q, q, q, q, big, None) == -1 and b"N=0" in err()
    for i in (1, 2, 5, 6, 7, 8, 9, 10, 11, 12):
        args = [h, q, q, 2, 0, q, q, q, q, q, q, q, q, q, big, None]
        args[i] = None
        assert L.sdfr_vae_trainer_backward(*args) == -2 and b"NULL pointer" in err(), i
    assert L.sdfr_vae_trainer_backward(h, q, q, 2, 0, q, q, q, q, q, q, q, q, None, big, None) == -2
    assert L.sdfr_vae_trainer_backward(h, q, q, 2, 0, q, q, q, q, q, q, q, q, q, 100, None) == -3 and b"workspace" in err()
    # the size queries
    assert L.sdfr_vae_trainer_tape_bytes(None, 2) == 0 and L.sdfr_vae_trainer_tape_bytes(h, 0) == 0
    assert L.sdfr_vae_trainer_workspace_bytes(None, 2) == 0 and L.sdfr_vae_trainer_workspace_bytes(h, 0) == 0
    assert L.sdfr_vae_trainer_param_count(None) == 0
    assert L.sdfr_vae_trainer_workspace_bytes(h, 3) > L.sdfr_vae_trainer_workspace_bytes(h, 2)
    L.sdfr_vae_trainer_destroy(h)
    L.sdfr_vae_trainer_destroy(None)
    # Adam
    assert L.sdfr_adam_flat(None, q, q, q, q, 4, 1e-3, 0, None) == -2 and b"sdfr_adam_flat" in err()
    assert L.sdfr_adam_flat(q, q, q, q, None, 4, 1e-3, 0, None) == -2
    assert L.sdfr_adam_flat(q, q, q, q, q, 0, 1e-3, 0, None) == -1 and b"n=0" in err()
    assert L.sdfr_adam_flat(q, q, q, q, q, 4, -1.0, 0, None) == -1 and b"lr" in err()
    # creation: the inference handles' checks and messages
    create(L, tw.T16, -1, latent=0)
    assert b"latent size 0" in err()
    create(L, tw.T16, -1, cout=[6, 4, 2])
    assert b"last conv layer must have one output channel" in err()
    create(L, tw.T16, -1, fc=[10, 127])
    assert b"last fc layer (127) does not match the first conv input" in err()
    create(L, tw.T16, -1, cin=[2, 5, 4])
    assert b"conv layer 0 out_channels != next in_channels" in err()
    ops = [[1, 1, 3, 3, 2, 0, 1, 0], [9, 0, 0, 0, 0, 0, 0, 0]]
    create(L, tw.T16, -1, ops=ops)
    assert b"op 1: unknown op type 9" in err()
    ops = [[1, 2, 3, 3, 2, 0, 1, 0]]
    create(L, tw.T16, -1, ops=ops)
    assert b"op 0: in_channels 2, but the input has 1 channels" in err()
    create(L, tw.T16, -1, tsdf=-0.5)
    assert b"tsdf" in err()


def test_trainer_rejects_what_is_not_implemented():
    """before anything touches the GPU"""
    from sdfest_amd import SDFVAETrainer
    with pytest.raises(NotImplementedError, match="pc_weight"):
        SDFVAETrainer(dict(tw.T16, pc_weight=1.0))
    bad = dict(tw.T16, encoder={"layer_infos": [tw.layer("Conv3d", in_channels=1, out_channels=3, kernel_size=3),
                                                tw.layer("BatchNorm3d", num_features=3), tw.layer("Flatten")]})
    with pytest.raises(ValueError, match="layer 1: type 'torch.nn.BatchNorm3d' is not supported"):
        SDFVAETrainer(bad)
    bad = dict(tw.T16, encoder={"layer_infos": [tw.layer("Conv3d", in_channels=1, out_channels=3, kernel_size=3, dilation=2),
                                                tw.layer("Flatten")]})
    with pytest.raises(ValueError, match=r"layer 0 \(torch.nn.Conv3d\): dilation=2 is not supported"):
        SDFVAETrainer(bad)
    with pytest.raises(KeyError, match="latent_size"):
        SDFVAETrainer({"encoder": tw.T16["encoder"], "decoder": tw.T16["decoder"]})


def test_initial_state_is_torchs_default_and_seeded():
    from sdfest_amd.train import initial_state, parameter_shapes
    a, b, c = initial_state(tw.T16, 4), initial_state(tw.T16, 4), initial_state(tw.T16, 5)
    assert [k for k, _ in parameter_shapes(tw.T16)] == list(a)
    assert all(torch.equal(a[k], b[k]) for k in a) and not all(torch.equal(a[k], c[k]) for k in a)
    for key, bound in (("encoder._features.2.weight", 1 / np.sqrt(81)), ("encoder._features.2.bias", 1 / np.sqrt(81)),
                       ("decoder._fc_layers.1.weight", 1 / np.sqrt(10)), ("encoder.linear_means.bias", 1 / np.sqrt(12))):
        t = a[key]
        assert t.dtype == torch.float32 and float(t.abs().max()) <= bound
        if t.numel() >= 100:
            assert float(t.abs().max()) > 0.9 * bound and abs(float(t.mean())) < 0.2 * bound


def test_checkpoint_file_round_trips(tmp_path):
    from sdfest_amd.train import read_checkpoint, write_checkpoint
    g = torch.Generator().manual_seed(0)
    ck = {"params": torch.rand(100, generator=g), "exp_avg": torch.rand(100, generator=g),
          "exp_avg_sq": torch.rand(100, generator=g), "adam_step": 7, "iteration": 7, "seed": 3,
          "config": dict(tw.T16), "keys": ["encoder.a", "decoder.b"]}
    path = str(tmp_path / "t.ckpt")
    write_checkpoint(path, ck)
    back = read_checkpoint(path)
    assert sorted(back) == sorted(ck)
    for k, v in ck.items():
        assert torch.equal(back[k], v) if isinstance(v, torch.Tensor) else back[k] == v, k
    torch.save({"params": ck["params"]}, path)
    with pytest.raises(ValueError, match="not a trainer checkpoint"):
        read_checkpoint(path)


def test_train_vae_help_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_vae.py"), "--help"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in ("--config", "--dataset_path", "--out", "--checkpoint", "--iterations", "--batch_size", "--seed"):
        assert flag in out.stdout
