"""CPU: the VAE encoder's host side -- layer parsing and output sizes, the reference's state-dict keys, rejection of
what the kernels do not implement, C-ABI argument errors (checked before any HIP call), the noise twin pinned to known
values, and the reference golden (tests/golden/encoder_mug.npz) reproduced by the layers in float64 torch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import encoder_twin as et
from helpers import GOLDEN


def conv(cin, cout, k, **kw):
    return {"type": "torch.nn.Conv3d", "args": {"in_channels": cin, "out_channels": cout, "kernel_size": k, **kw}}


RELU = {"type": "torch.nn.ReLU", "args": {}}
FLAT = {"type": "torch.nn.Flatten", "args": {}}


def test_mug_layers_parse():
    from sdfest_amd.vae import parse_encoder_layers
    p = parse_encoder_layers(64, et.MUG_ENCODER["layer_infos"])
    # Conv3d(s=2) + ReLU x 3 + Flatten: 64 -> 31 -> 15 -> 7, 16 * 7^3 features; ReLUs fused into the convolutions
    assert p["ops"] == [[1, 1, 4, 3, 2, 0, 1, 0], [1, 4, 8, 3, 2, 0, 1, 0], [1, 8, 16, 3, 2, 0, 1, 0]]
    assert p["shapes"] == [(4, 31, 31, 31)] * 2 + [(8, 15, 15, 15)] * 2 + [(16, 7, 7, 7)] * 2 + [(5488,)]
    assert p["features"] == 5488 and p["params"] == [0, 2, 4]


def test_big_1_relu_layers_parse():
    from sdfest_amd.vae import parse_encoder_layers
    p = parse_encoder_layers(64, et.BIG_1_RELU_ENCODER["layer_infos"])
    assert [op[0] for op in p["ops"]] == [1, 2, 1, 2, 1, 2, 3]
    assert p["shapes"][2] == (8, 32, 32, 32) and p["shapes"][8] == (16, 8, 8, 8) and p["shapes"][-1] == (128,)
    assert p["features"] == 128 and p["params"] == [0, 3, 6, 10]
    assert p["ops"][-1] == [3, 8192, 128, 0, 0, 0, 1, 0]


@pytest.mark.parametrize("layers,shape", [
    ([conv(1, 3, 5, stride=3, padding=2)], (3, 7, 7, 7)),                       # (19 + 4 - 5) // 3 + 1
    ([conv(1, 2, [3, 3, 3], stride=(2, 2, 2), padding="valid")], (2, 9, 9, 9)),
    ([{"type": "torch.nn.MaxPool3d", "args": {"kernel_size": 3}}], (1, 6, 6, 6)),   # stride defaults to kernel
    ([{"type": "torch.nn.MaxPool3d", "args": {"kernel_size": 2, "stride": 1}}], (1, 18, 18, 18)),
    ([RELU, conv(1, 1, 1)], (1, 19, 19, 19)),
])
def test_output_size_inference(layers, shape):
    from sdfest_amd.vae import parse_encoder_layers
    p = parse_encoder_layers(19, layers + [FLAT])
    assert p["shapes"][len(layers) - 1] == shape
    assert p["features"] == int(np.prod(shape))
    # the same sizes as torch's own modules
    mods = [getattr(torch.nn, l["type"].rsplit(".", 1)[-1])(**l["args"]) for l in layers]
    assert tuple(torch.nn.Sequential(*mods)(torch.zeros(1, 1, 19, 19, 19)).shape[1:]) == shape


def test_leading_relu_is_an_op_and_repeated_relu_fuses():
    from sdfest_amd.vae import parse_encoder_layers
    p = parse_encoder_layers(9, [RELU, RELU, conv(1, 2, 3), RELU, RELU, FLAT,
                                 {"type": "torch.nn.Linear", "args": {"in_features": 686, "out_features": 5}}])
    assert p["ops"] == [[4, 0, 0, 0, 0, 0, 1, 0], [1, 1, 2, 3, 1, 0, 1, 0], [3, 686, 5, 0, 0, 0, 0, 0]]
    assert p["params"] == [2, 6]


def test_state_dict_keys_and_prefix():
    from sdfest_amd.vae import _encoder_params, encoder_state_keys, parse_encoder_layers
    p = parse_encoder_layers(64, et.MUG_ENCODER["layer_infos"])
    keys = encoder_state_keys(p)
    assert keys == ["encoder._features.0.weight", "encoder._features.0.bias", "encoder._features.2.weight",
                    "encoder._features.2.bias", "encoder._features.4.weight", "encoder._features.4.bias",
                    "encoder.linear_means.weight", "encoder.linear_means.bias", "encoder.linear_log_var.weight",
                    "encoder.linear_log_var.bias"]
    g = np.load(os.path.join(GOLDEN, "encoder_mug.npz"))
    state = {k: g[k] for k in keys}
    flat = _encoder_params(p, 8, state, "encoder.")
    assert flat.size == 92280 == sum(state[k].size for k in keys)
    bare = {k[len("encoder."):]: v for k, v in state.items()}
    assert np.array_equal(_encoder_params(p, 8, bare, ""), flat)
    bad = dict(state)
    bad["encoder.linear_means.weight"] = np.zeros((8, 5487), np.float32)
    with pytest.raises(ValueError, match="linear_means.weight"):
        _encoder_params(p, 8, bad, "encoder.")
    del bad["encoder._features.2.bias"]
    with pytest.raises(KeyError, match="_features.2.bias"):
        _encoder_params(p, 8, bad, "encoder.")


@pytest.mark.parametrize("layer,match", [
    (conv(1, 2, 3, dilation=2), r"layer 0 \(torch.nn.Conv3d\): dilation"),
    (conv(1, 2, 3, groups=2), r"layer 0 .*groups"),
    (conv(1, 2, (3, 3, 1)), r"layer 0 .*kernel_size.*not cubic"),
    (conv(1, 2, 3, stride=(1, 2, 2)), r"layer 0 .*stride.*not cubic"),
    (conv(1, 2, 3, padding="same"), r"layer 0 .*padding"),
    (conv(1, 2, 3, padding_mode="reflect"), r"layer 0 .*padding_mode"),
    (conv(1, 2, 3, bias=False), r"layer 0 .*bias"),
    (conv(2, 2, 3), r"layer 0 .*in_channels=2"),
    ({"type": "torch.nn.LeakyReLU", "args": {}}, r"layer 0: type 'torch.nn.LeakyReLU'"),
    ({"type": "torch.nn.Conv2d", "args": {}}, r"layer 0: type"),
    ({"type": "torch.nn.MaxPool3d", "args": {"kernel_size": 2, "padding": 1}}, r"layer 0 .*padding"),
    ({"type": "torch.nn.MaxPool3d", "args": {"kernel_size": 2, "ceil_mode": True}}, r"layer 0 .*ceil_mode"),
    ({"type": "torch.nn.MaxPool3d", "args": {"kernel_size": 2, "dilation": 2}}, r"layer 0 .*dilation"),
    ({"type": "torch.nn.ReLU", "args": {"negative_slope": 0.1}}, r"layer 0 .*negative_slope"),
    ({"type": "torch.nn.Linear", "args": {"in_features": 1000, "out_features": 4}}, r"layer 0 .*flat input"),
])
def test_unsupported_layers_are_rejected(layer, match):
    from sdfest_amd.vae import parse_encoder_layers
    with pytest.raises(ValueError, match=match):
        parse_encoder_layers(10, [layer, FLAT])


def test_rejections_name_the_layer_index():
    from sdfest_amd.vae import parse_encoder_layers
    with pytest.raises(ValueError, match=r"layer 2 \(torch.nn.Conv3d\): dilation"):
        parse_encoder_layers(16, [conv(1, 2, 3), RELU, conv(2, 2, 3, dilation=2), FLAT])
    with pytest.raises(ValueError, match=r"layer 3 .*in_features=10"):
        parse_encoder_layers(4, [conv(1, 2, 3), RELU, FLAT,
                                 {"type": "torch.nn.Linear", "args": {"in_features": 10, "out_features": 3}}])
    with pytest.raises(ValueError, match="end flat"):
        parse_encoder_layers(8, [conv(1, 2, 3)])


def test_encoder_rejects_before_touching_the_device():
    from sdfest_amd import SDFEncoder, SDFVAE
    with pytest.raises(ValueError, match="dilation"):
        SDFEncoder(16, 4, [conv(1, 2, 3, dilation=2), FLAT], state_dict={}, device="cuda")
    with pytest.raises(ValueError, match="state_dict"):
        SDFEncoder(16, 4, [conv(1, 2, 3), FLAT], state_dict=None)
    with pytest.raises(ValueError, match="LeakyReLU"):
        SDFVAE(16, 4, {"layer_infos": [{"type": "torch.nn.LeakyReLU", "args": {}}, FLAT]},
               {"fc_layers": [], "conv_layers": []}, state_dict={})


# ---- C ABI: argument errors are reported before any HIP call (no GPU here) --------------------------------------------
def _ops(rows):
    a = np.ascontiguousarray(np.array(rows, dtype=np.int32).reshape(-1, 8))
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_cabi_encoder_argument_errors():
    from sdfest_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    prm = np.zeros(10, np.float32)
    P = prm.ctypes.data_as(ctypes.c_void_p)

    def create(ops, n_params=prm.size, volume=8, latent=2, params=P):
        a, p = _ops(ops)
        return L.sdfr_encoder_create(params, n_params, volume, latent, a.shape[0], p, 0, ctypes.byref(h))

    def err():
        return L.sdfr_last_error().decode()

    assert create([[1, 1, 2, 3, 1, 0, 0, 0]], params=None) == -2
    assert create([[9, 1, 2, 3, 1, 0, 0, 0]]) == -1 and "op 0: unknown op type 9" in err()
    assert create([[1, 1, 2, 3, 1, 0, 0, 0], [1, 3, 2, 3, 1, 0, 0, 0]]) == -1 and "op 1: in_channels 3" in err()
    assert create([[1, 1, 2, 9, 1, 0, 0, 0]]) == -1 and "op 0: kernel_size 9" in err()
    assert create([[1, 1, 2, 3, 0, 0, 0, 0]]) == -1 and "op 0: stride 0" in err()
    assert create([[2, 0, 0, 2, 2, 1, 0, 0]]) == -1 and "op 0: padding 1" in err()
    assert create([[3, 100, 4, 0, 0, 0, 0, 0]]) == -1 and "op 0: in_features 100" in err()
    assert create([[3, 512, 4, 0, 0, 0, 0, 0], [1, 4, 4, 1, 1, 0, 0, 0]]) == -1 and "op 1" in err()
    assert create([[1, 1, 2, 3, 1, 0, 0, 0]], latent=0) == -1
    assert create([[1, 1, 2, 3, 1, 0, 0, 0]], volume=0) == -1
    # 2 * 1 * 27 + 2 = 56 convolution parameters, heads 2 * (2 * 2 * 6^3 + 2) = 1732: anything else is a count mismatch
    assert create([[1, 1, 2, 3, 1, 0, 1, 0]]) == -1 and "parameter count 10" in err() and "(1788)" in err()
    assert L.sdfr_encoder_workspace_bytes(None, 4) == 0
    buf = ctypes.c_void_p(16)
    assert L.sdfr_encoder_forward(None, buf, 1, buf, buf, None, 0, None, 0, None) == -2


def test_cabi_sample_and_clamp_argument_errors():
    from sdfest_amd import _lib
    L = _lib.lib()
    buf = ctypes.c_void_p(16)
    assert L.sdfr_normal_sample(buf, -1, 8, 0, 0, None) == -1
    assert L.sdfr_normal_sample(buf, 4, 0, 0, 0, None) == -1
    assert L.sdfr_normal_sample(None, 4, 8, 0, 0, None) == -2
    assert L.sdfr_normal_sample(None, 0, 8, 0, 0, None) == 0          # nothing to do: no HIP call either
    assert L.sdfr_clamp(buf, 16, -0.5, 0, None) == -1
    assert L.sdfr_clamp(None, 16, 0.5, 0, None) == -2
    assert L.sdfr_clamp(None, 0, 0.5, 0, None) == 0


# ---- the noise ------------------------------------------------------------------------------------------------------
def test_noise_twin_pinned():
    e = et.normal_eps(1234, 3, 4)
    np.testing.assert_array_equal(e, np.array([
        [0.7969977, 0.2501745, -1.6083478, 0.4279791],
        [-0.99386835, 0.21844324, 0.8512204, -0.6671857],
        [0.3233755, 0.5710488, -0.53501475, -0.04014368]], np.float32))
    np.testing.assert_array_equal(et.normal_eps(0, 1, 2), np.array([[-1.9888095, 0.16926055]], np.float32))
    np.testing.assert_array_equal(et.normal_eps(2 ** 64 - 1, 1, 2), np.array([[0.6063843, 0.05340161]], np.float32))
    # depends on (seed, i, j) only: a prefix of rows, a prefix of columns
    big = et.normal_eps(99, 50, 16)
    assert np.array_equal(big[:7], et.normal_eps(99, 7, 16))
    assert np.array_equal(big[:, :5], et.normal_eps(99, 50, 5))
    x = et.normal_eps(7, 4096, 8).astype(np.float64)
    assert abs(x.mean()) < 0.01 and abs(x.std() - 1) < 0.01


def test_noise_twin_uses_the_pinned_philox():
    import metrics_twin as mt
    # Random123's known-answer vector for Philox-4x32-10 (ctr = key = 0)
    w = mt.philox4x32_10(np.zeros((1, 4), np.uint32), (np.uint32(0), np.uint32(0)))
    assert [int(v) for v in w[0]] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


# ---- the golden, in float64 -------------------------------------------------------------------------------------------
def golden_inputs(g):
    from sdfest_amd.synthetic import blobs_sdf, sphere_sdf
    z0 = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))["z0_full"].astype(np.float32)
    make = {"z0": lambda: z0, "sphere": lambda: sphere_sdf(0.5)}
    out = []
    for n in g["names"]:
        n = str(n)
        out.append(make[n]() if n in make else blobs_sdf(int(n[len("blobs"):])))
    return np.stack(out)[:, None]


def test_golden_reproduced_in_float64():
    g = np.load(os.path.join(GOLDEN, "encoder_mug.npz"))
    x = golden_inputs(g)
    m, lv = et.torch_encoder(g, et.MUG_ENCODER["layer_infos"], x)
    for got, ref in ((m.numpy(), g["means"]), (lv.numpy(), g["log_var"])):
        assert np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-5), np.max(np.abs(got - ref))
    xt = np.clip(golden_inputs({"names": np.array(["blobs0"])}), -g["tsdf"], g["tsdf"])
    m, lv = et.torch_encoder(g, et.MUG_ENCODER["layer_infos"], xt)
    assert np.all(np.abs(m.numpy() - g["tsdf_means"]) <= 1e-4 * np.abs(g["tsdf_means"]) + 1e-5)
    assert np.all(np.abs(lv.numpy() - g["tsdf_log_var"]) <= 1e-4 * np.abs(g["tsdf_log_var"]) + 1e-5)
    # the inputs differ from each other, so do their codes
    assert len({tuple(np.round(r, 4)) for r in g["means"]}) == len(g["names"])
