"""GPU: seeded random encoders -- Conv3d with kernels 1 / 3 / 5, strides 1 ... 3, padding 0 ... 2 and 1 ... 24 channels,
optional MaxPool3d and Linear layers, volumes 9 ... 64, batches 1 ... 40, latent sizes 1 ... 16 -- against the layers
written out in float64 torch on the CPU (tests/encoder_twin.py).  Which ops run over global memory and which in the
one-workgroup-per-sample chain depends on the activation sizes, and this file walks those choices."""
import os

import numpy as np
import pytest
import torch

import encoder_twin as et

pytestmark = pytest.mark.gpu


def draw(seed):
    rng = np.random.default_rng(7000 + seed)
    D = int(rng.integers(9, 65))
    L = int(rng.integers(1, 17))
    N = int(rng.integers(1, 41))
    layers, C, S, macs = [], 1, D, 0
    for _ in range(int(rng.integers(1, 4))):
        k = int(rng.choice([1, 3, 5]))
        p = int(rng.integers(0, 3))
        s = int(rng.integers(1, 4))
        if S + 2 * p < k:
            continue
        cout = int(rng.integers(1, 25))
        if C * cout * k ** 3 > 6000:       # keep the float64 reference quick
            cout = max(1, 6000 // (C * k ** 3))
        layers.append({"type": "torch.nn.Conv3d", "args": {"in_channels": C, "out_channels": cout, "kernel_size": k,
                                                          "stride": s, "padding": p}})
        C, S = cout, (S + 2 * p - k) // s + 1
        macs += layers[-1]["args"]["in_channels"] * cout * k ** 3 * S ** 3
        if rng.random() < 0.7:
            layers.append({"type": "torch.nn.ReLU", "args": {}})
        if S >= 2 and rng.random() < 0.4:
            pk = int(rng.integers(1, min(S, 3) + 1))
            ps = int(rng.integers(1, 3))
            layers.append({"type": "torch.nn.MaxPool3d", "args": {"kernel_size": pk, "stride": ps}})
            S = (S - pk) // ps + 1
    layers.append({"type": "torch.nn.Flatten", "args": {}})
    F = C * S ** 3
    if F <= 40000 and rng.random() < 0.5:
        out = int(rng.integers(1, 65))
        layers.append({"type": "torch.nn.Linear", "args": {"in_features": F, "out_features": out}})
        if rng.random() < 0.5:
            layers.append({"type": "torch.nn.ReLU", "args": {}})
    return D, L, max(1, min(N, int(2e9 // max(macs, 1)))), layers   # (the float64 reference's time)


@pytest.mark.parametrize("seed", range(int(os.environ.get("SDFR_FUZZ_SEEDS", "16"))))
def test_random_encoder_against_float64(seed):
    from sdfest_amd import SDFEncoder
    from sdfest_amd.vae import parse_encoder_layers
    D, L, N, layers = draw(seed)
    state = et.random_state(parse_encoder_layers(D, layers), L, seed=seed)
    enc = SDFEncoder(D, L, layers, state_dict=state)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, 1, D, D, D)).astype(np.float32)
    with torch.no_grad():
        m, lv = enc(torch.tensor(x, device="cuda"))
        m1, lv1 = enc(torch.tensor(x[-1:], device="cuda"))
    assert torch.equal(m1[0], m[-1]) and torch.equal(lv1[0], lv[-1])
    m64, lv64 = et.torch_encoder(state, layers, x)
    for got, ref in ((m.cpu().numpy(), m64.numpy()), (lv.cpu().numpy(), lv64.numpy())):
        scale = max(np.abs(ref).max(), 1e-3)
        err = np.abs(got - ref)
        assert np.all(err <= 1e-5 * np.abs(ref) + 1e-5 * scale), (layers, err.max(), scale)
