"""CPU twins of sdfest_amd/csrc/encoder.hip: the noise (Philox-4x32-10 from metrics_twin + Box-Muller in fp64) and the
encoder's layers written out in torch (float64 on the CPU: the layer sequence of sdf_vae.py:103-152)."""
import numpy as np
import torch
import torch.nn.functional as F

from metrics_twin import philox4x32_10

NOISE_STREAM = 0x56414531

MUG_ENCODER = {"layer_infos": [          # tests/initilization/vae_model/mug.yaml of the reference, key encoder
    {"type": "torch.nn.Conv3d", "args": {"in_channels": 1, "out_channels": 4, "kernel_size": 3, "stride": 2}},
    {"type": "torch.nn.ReLU", "args": {}},
    {"type": "torch.nn.Conv3d", "args": {"in_channels": 4, "out_channels": 8, "kernel_size": 3, "stride": 2}},
    {"type": "torch.nn.ReLU", "args": {}},
    {"type": "torch.nn.Conv3d", "args": {"in_channels": 8, "out_channels": 16, "kernel_size": 3, "stride": 2}},
    {"type": "torch.nn.ReLU", "args": {}},
    {"type": "torch.nn.Flatten", "args": {}}]}

BIG_1_RELU_ENCODER = {"layer_infos": [   # sdfest/vae/configs/big_1_relu.yaml of the reference, key encoder
    {"type": "torch.nn.Conv3d", "args": {"in_channels": 1, "out_channels": 8, "kernel_size": 3, "padding": 1}},
    {"type": "torch.nn.ReLU", "args": {}},
    {"type": "torch.nn.MaxPool3d", "args": {"kernel_size": 2, "stride": 2}},
    {"type": "torch.nn.Conv3d", "args": {"in_channels": 8, "out_channels": 16, "kernel_size": 3, "padding": 1}},
    {"type": "torch.nn.ReLU", "args": {}},
    {"type": "torch.nn.MaxPool3d", "args": {"kernel_size": 2, "stride": 2}},
    {"type": "torch.nn.Conv3d", "args": {"in_channels": 16, "out_channels": 16, "kernel_size": 3, "padding": 1}},
    {"type": "torch.nn.ReLU", "args": {}},
    {"type": "torch.nn.MaxPool3d", "args": {"kernel_size": 2, "stride": 2}},
    {"type": "torch.nn.Flatten", "args": {}},
    {"type": "torch.nn.Linear", "args": {"in_features": 8192, "out_features": 128}},
    {"type": "torch.nn.ReLU", "args": {}}]}


def normal_eps(seed, n, L):
    """eps [n][L] float32: counter {i, j, 0, NOISE_STREAM}, key = seed; Box-Muller in fp64, rounded once"""
    i, j = np.meshgrid(np.arange(n, dtype=np.uint32), np.arange(L, dtype=np.uint32), indexing="ij")
    ctr = np.zeros((n, L, 4), dtype=np.uint32)
    ctr[..., 0], ctr[..., 1], ctr[..., 3] = i, j, NOISE_STREAM
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(ctr, (np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)))
    u1 = ((w[..., 0] >> 5).astype(np.float64) * 67108864.0 + (w[..., 1] >> 6).astype(np.float64)) / 9007199254740992.0
    u2 = ((w[..., 2] >> 5).astype(np.float64) * 67108864.0 + (w[..., 3] >> 6).astype(np.float64)) / 9007199254740992.0
    return (np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)).astype(np.float32)


def torch_encoder(state, layer_infos, x, dtype=torch.float64, prefix="encoder."):
    """(means, log_var) of the reference's layer sequence, on the CPU in `dtype`"""
    def p(name):
        return torch.as_tensor(np.asarray(state[prefix + name]), dtype=dtype)
    h = torch.as_tensor(np.asarray(x), dtype=dtype)
    for i, info in enumerate(layer_infos):
        t, a = info["type"].rsplit(".", 1)[-1], info.get("args", {})
        if t == "Conv3d":
            h = F.conv3d(h, p(f"_features.{i}.weight"), p(f"_features.{i}.bias"), stride=a.get("stride", 1),
                         padding=a.get("padding", 0))
        elif t == "ReLU":
            h = torch.relu(h)
        elif t == "MaxPool3d":
            h = F.max_pool3d(h, a["kernel_size"], a.get("stride"))
        elif t == "Flatten":
            h = h.flatten(1)
        elif t == "Linear":
            h = F.linear(h, p(f"_features.{i}.weight"), p(f"_features.{i}.bias"))
        else:
            raise ValueError(t)
    return (F.linear(h, p("linear_means.weight"), p("linear_means.bias")),
            F.linear(h, p("linear_log_var.weight"), p("linear_log_var.bias")))


def random_state(plan, latent, seed):
    """seeded He-scaled weights and small biases with the reference's keys for a parsed encoder"""
    from sdfest_amd.vae import ENC_CONV, ENC_LINEAR, encoder_state_keys
    rng = np.random.default_rng(seed)
    shapes = []
    for op in plan["ops"]:
        if op[0] == ENC_CONV:
            shapes += [(op[2], op[1], op[3], op[3], op[3]), (op[2],)]
        elif op[0] == ENC_LINEAR:
            shapes += [(op[2], op[1]), (op[2],)]
    shapes += [(latent, plan["features"]), (latent,)] * 2
    state = {}
    for key, shape in zip(encoder_state_keys(plan), shapes):
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        scale = np.sqrt(2.0 / fan_in) if len(shape) > 1 else 0.05
        state[key] = (rng.standard_normal(shape) * scale).astype(np.float32)
    return state
