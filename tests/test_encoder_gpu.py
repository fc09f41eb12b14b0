"""GPU: the VAE encoder (sdfest_amd.SDFEncoder / SDFVAE over csrc/encoder.hip) -- the mug encoder against the
reference's golden and float64 torch, big_1_relu with seeded weights, batch invariance and determinism, the noise
against its twin, SDFVAE's methods, prepare_input, the grad-mode error, and the evaluation chain
encode -> decode -> mesh -> chamfer."""
import os

import numpy as np
import pytest
import torch

import encoder_twin as et
import test_decoder_gpu as D
from helpers import GOLDEN
from test_encoder_cpu import golden_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    g = np.load(os.path.join(GOLDEN, "encoder_mug.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def vae(G):
    from sdfest_amd import SDFVAE
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    w = np.load(os.path.join(GOLDEN, "mug_decoder_weights.npz"))
    state = {k: w[k] for k in w.files}
    state.update({k: v for k, v in G.items() if k.startswith("encoder.")})
    cfg = D.mug_config(d)
    cfg["encoder"] = et.MUG_ENCODER
    return SDFVAE.from_config(cfg, state)


@pytest.fixture(scope="module")
def X(G):
    return torch.tensor(golden_inputs(G), device="cuda")


def close(got, ref, rtol, atol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    assert np.all(err <= rtol * np.abs(ref) + atol), (err.max(), (err / (rtol * np.abs(ref) + atol)).max())
    return (err / (rtol * np.abs(ref) + atol)).max()


def test_mug_matches_reference_golden_and_float64(vae, G, X):
    with torch.no_grad():
        m, lv = vae.encoder(X)
    assert m.shape == lv.shape == (X.shape[0], 8)
    close(m.cpu(), G["means"], 1e-4, 1e-5)
    close(lv.cpu(), G["log_var"], 1e-4, 1e-5)
    m64, lv64 = et.torch_encoder(G, et.MUG_ENCODER["layer_infos"], X.cpu().numpy())
    # observed on MI355X: the largest error is ~0.05 of this bound (fixed-order fp32 sums)
    used = max(close(m.cpu(), m64.numpy(), 1e-5, 1e-5), close(lv.cpu(), lv64.numpy(), 1e-5, 1e-5))
    print(f"mug vs float64: {used:.3f} of the 1e-5 + 1e-5 bound")


def test_prepare_input_in_place_then_encode(G):
    from sdfest_amd import SDFEncoder
    from sdfest_amd.synthetic import blobs_sdf
    enc = SDFEncoder(64, 8, et.MUG_ENCODER["layer_infos"], tsdf=float(G["tsdf"]), state_dict=G)
    x = torch.tensor(blobs_sdf(0)[None, None], device="cuda")
    ptr, raw = x.data_ptr(), x.clone()
    enc.prepare_input(x)
    assert x.data_ptr() == ptr
    assert torch.equal(x, raw.clamp(-float(G["tsdf"]), float(G["tsdf"])))
    assert (raw.abs() > float(G["tsdf"])).any()
    with torch.no_grad():
        m, lv = enc(x)
    close(m.cpu(), G["tsdf_means"], 1e-4, 1e-5)
    close(lv.cpu(), G["tsdf_log_var"], 1e-4, 1e-5)
    plain = SDFEncoder(64, 8, et.MUG_ENCODER["layer_infos"], state_dict=G)   # tsdf=False: no clamp
    plain.prepare_input(raw)
    assert not torch.equal(raw, x)


def test_big_1_relu_seeded_against_float64():
    from sdfest_amd import SDFEncoder
    from sdfest_amd.vae import parse_encoder_layers
    layers = et.BIG_1_RELU_ENCODER["layer_infos"]
    state = et.random_state(parse_encoder_layers(64, layers), 16, seed=5)
    enc = SDFEncoder(64, 16, layers, state_dict=state)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 1, 64, 64, 64)).astype(np.float32)
    with torch.no_grad():
        m, lv = enc(torch.tensor(x, device="cuda"))
    m64, lv64 = et.torch_encoder(state, layers, x)
    close(m.cpu(), m64.numpy(), 1e-5, 1e-5)
    close(lv.cpu(), lv64.numpy(), 1e-5, 1e-5)


def test_batch_invariance_and_determinism(vae, X):
    with torch.no_grad():
        m, lv = vae.encoder(X)
        perm = torch.randperm(X.shape[0], generator=torch.Generator().manual_seed(1)).cuda()
        mp, lvp = vae.encoder(X[perm])
        assert torch.equal(mp, m[perm]) and torch.equal(lvp, lv[perm])
        for i in range(X.shape[0]):
            mi, lvi = vae.encoder(X[i:i + 1])
            assert torch.equal(mi[0], m[i]) and torch.equal(lvi[0], lv[i])
        big = X.repeat(5, 1, 1, 1, 1)                       # 35 rows: the same bits in every copy
        mb, lvb = vae.encoder(big)
        assert torch.equal(mb, m.repeat(5, 1)) and torch.equal(lvb, lv.repeat(5, 1))
        for _ in range(3):
            m2, lv2 = vae.encoder(X)
            assert torch.equal(m2, m) and torch.equal(lv2, lv)


def test_z_matches_the_noise_twin_and_prefix(vae, X):
    with torch.no_grad():
        z, m, lv = vae.encode(X, seed=1234)
    eps = torch.tensor(et.normal_eps(1234, X.shape[0], 8))
    ref = eps * torch.exp(0.5 * lv.cpu()) + m.cpu()
    assert torch.allclose(z.cpu(), ref, rtol=1e-6, atol=1e-7)
    z3, m3, _ = vae.encode(X[:3], seed=1234)
    assert torch.equal(z3, z[:3]) and torch.equal(m3, m[:3])
    z_other, _, _ = vae.encode(X, seed=1235)
    assert not torch.equal(z_other, z)
    torch.manual_seed(7)
    a = vae.encode(X)[0]
    torch.manual_seed(7)
    assert torch.equal(vae.encode(X)[0], a)


def test_sample_moments_and_twin(vae):
    s = vae.sample(4096, seed=7)
    assert s.shape == (4096, 8) and s.is_cuda
    tw = et.normal_eps(7, 4096, 8)
    assert np.allclose(s.cpu().numpy(), tw, rtol=1e-6, atol=1e-7)
    v = s.double()
    assert abs(v.mean().item()) < 0.02 and abs(v.std().item() - 1) < 0.02
    assert abs(((v - v.mean()) ** 3).mean().item()) < 0.1 and abs((v ** 4).mean().item() - 3) < 0.2
    assert torch.equal(vae.sample(10, seed=7), s[:10])
    recon, z = vae.inference(n=2, seed=3)
    assert recon.shape == (2, 1, 64, 64, 64) and torch.equal(z, vae.sample(2, seed=3))
    assert torch.equal(recon, vae.decode(z))


def test_forward_recon_is_decoder_of_z(vae, X):
    with torch.no_grad():
        recon, m, lv, z = vae(X[:3], seed=11)
        z2, m2, lv2 = vae.encode(X[:3], seed=11)
        assert torch.equal(z, z2) and torch.equal(m, m2) and torch.equal(lv, lv2)
        assert torch.equal(recon, vae.decoder(z))
        assert torch.equal(vae.forward(X[:3], enforce_tsdf=True, seed=11)[0], vae.decode(z, enforce_tsdf=True))


def test_input_checks_and_grad_mode(vae, X):
    x = X[:1].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        vae.encode(x)
    with pytest.raises(NotImplementedError):
        vae.encoder(x)
    with torch.no_grad():
        vae.encoder(x)                                   # no grad mode: fine
    for bad in (X[:1].double(), X[:1].cpu(), X[:1, :, :32], X[0], X[:0], X[:1].expand(1, 2, 64, 64, 64)):
        with pytest.raises(RuntimeError):
            vae.encoder(bad)


def test_chain_encode_decode_mesh_chamfer_batched_equals_single(vae):
    from sdfest_amd import extract_mesh, reconstruction_metrics, sample_points, symmetric_chamfer
    z = torch.tensor(np.load(os.path.join(GOLDEN, "decoder_mug.npz"))["z"][:4], device="cuda")
    level = 0.0

    def chain(zs):
        with torch.no_grad():
            x = vae.decode(zs)                       # shapes the VAE can represent
            _, m, _ = vae.encode(x, seed=0)
            rec = vae.decode(m)
        gt_mesh, rec_mesh = extract_mesh(x, level), extract_mesh(rec, level)
        return m, sample_points(gt_mesh, 2000, seed=1), sample_points(rec_mesh, 2000, seed=2)

    m, gt, rc = chain(z)        # 4 latents: the decoder keeps its single-latent form (< 8), so rows match bitwise
    scores = reconstruction_metrics(gt, rc)["chamfer"]
    for k in range(4):
        mk, gk, rk = chain(z[k:k + 1])
        assert torch.equal(mk[0], m[k]) and torch.equal(gk[0], gt[k]) and torch.equal(rk[0], rc[k])
        c = symmetric_chamfer(gk[0], rk[0])
        assert c == scores[k].item()
        assert 0 < c < 0.05, c                       # the VAE reproduces its own shapes closely (the grid spans [-1, 1])
