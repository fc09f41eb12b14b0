"""GPU: training of the SDF VAE (sdfest_amd.SDFVAETrainer over csrc/vae_train.hip) against its float64 twin
(tests/vae_train_twin.py): every parameter gradient and the loss terms in both phases, the forward against the inference
handles, determinism, Adam against torch.optim.Adam, a 30-step trajectory across the phase switch, and the round trips
(state dict, checkpoint, fit, the command line).

Architectures: T16 / T8 (vae_train_twin: stride, padding, pool, an encoder Linear, a mid-network 1x1x1, odd resize ratios,
channel counts that are no multiple of 4; no final resize and no truncation) and the reference's mug model at N = 2."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import encoder_twin as et
import vae_train_twin as tw
from helpers import ROOT

pytestmark = pytest.mark.gpu

ARCH = {"T16": lambda: (tw.T16, tw.random_state(tw.T16, 11)), "T8": lambda: (tw.T8, tw.random_state(tw.T8, 12)),
        "mug": tw.mug_setup}
SEED = 5                                  # the golden's: eps = normal_eps(5, N, L)
PHASES = {"warm": 0, "post": 1001}        # iteration counters on the two sides of warm_up_iterations = 1000


@functools.lru_cache(maxsize=None)
def setup(arch):
    return ARCH[arch]()


@functools.lru_cache(maxsize=None)
def inputs(arch, N):
    return tw.blobs_at(setup(arch)[0]["sdf_size"], tuple(range(N)))


@functools.lru_cache(maxsize=None)
def reference(arch, N, phase):
    """the float64 twin's (terms, grads, (means, log_var, z, recon)): computed once, shared, never modified"""
    config, state = setup(arch)
    return tw.Twin(config, state).run(inputs(arch, N), et.normal_eps(SEED, N, config["latent_size"]), PHASES[phase])


@functools.lru_cache(maxsize=None)
def trainer(arch):
    from sdfest_amd import SDFVAETrainer
    config, state = setup(arch)
    return SDFVAETrainer(config, state)


def run(arch, N, phase):
    return trainer(arch).loss_and_grad(torch.tensor(inputs(arch, N), device="cuda"), seed=SEED, iteration=PHASES[phase])


def close(got, ref, rtol=1e-5, atol=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    used = np.abs(got - ref) / (rtol * np.abs(ref) + atol)
    assert np.all(used <= 1.0), used.max()
    return float(used.max())


CASES = [("T16", 1), ("T16", 3), ("T16", 8), ("T8", 2), ("mug", 2)]


@pytest.mark.parametrize("phase", list(PHASES))
@pytest.mark.parametrize("arch, N", CASES)
def test_gradients_and_loss_terms_match_float64_twin(arch, N, phase):
    """every element of every parameter's gradient within 1e-4 of the tensor's largest (the bound of the decoder's latent
    gradient, test_decoder_latent_gradient_matches_torch_autograd_golden; torch fp32 on the CPU stays within 3.5e-6 on
    the mug); the loss terms within 1e-5 relative + 1e-5 absolute (torch fp32 on the CPU: 3e-7).
    Observed on MI355X: the worst gradient element 3.0e-6 of its tensor's maximum (T16, N = 3, post phase,
    encoder._features.0.bias; the mug 2.0e-6 / 5.1e-7), the loss terms at most 0.031 of their bound."""
    terms, grads, _ = reference(arch, N, phase)
    out = run(arch, N, phase)
    worst, where = 0.0, None
    for name, g64 in grads.items():
        g = out["grads"][name].cpu().numpy().astype(np.float64)
        assert g.shape == g64.shape, name
        top = np.abs(g64).max()
        err = np.abs(g - g64).max() / top if top > 0 else np.abs(g).max()
        if err > worst:
            worst, where = err, name
    print(f"{arch} N={N} {phase}: worst gradient error {worst:.2e} of the tensor's maximum ({where})")
    used = max(close(out[k], terms[k]) for k in tw.TERMS)
    print(f"{arch} N={N} {phase}: loss terms use {used:.3f} of the 1e-5 + 1e-5 bound")
    assert worst <= 1e-4, f"{where}: {worst:.2e} of its maximum"


@pytest.mark.parametrize("arch, N", [("T16", 3), ("mug", 2)])
def test_forward_matches_twin_and_inference_handles(arch, N):
    """means, log_var, z and recon of the training forward and of SDFVAE.forward on handles built from state_dict(): both
    within 1e-5 + 1e-5 of the float64 twin; z is drawn from the same eps stream"""
    from sdfest_amd import SDFVAE
    config, _ = setup(arch)
    _, _, (m64, lv64, z64, r64) = reference(arch, N, "warm")
    out = run(arch, N, "warm")
    t = trainer(arch)
    vae = SDFVAE.from_config(config, t.state_dict(), sdf_size=config["sdf_size"])
    with torch.no_grad():
        recon, means, log_var, z = vae(torch.tensor(inputs(arch, N), device="cuda"), seed=SEED)
    for name, a, b, ref in (("means", out["means"], means, m64), ("log_var", out["log_var"], log_var, lv64),
                            ("z", out["z"], z, z64), ("recon", out["recon"], recon, r64)):
        print(f"{arch} {name}: trainer {close(a.cpu(), ref):.3f}, inference {close(b.cpu(), ref):.3f} of the bound")
    eps = torch.tensor(et.normal_eps(SEED, N, config["latent_size"]), device="cuda")
    assert torch.equal(out["z"], eps * torch.exp(0.5 * out["log_var"]) + out["means"])
    # the clamp of the post phase happens in the trainer's copy: the caller's tensor is left alone
    x = torch.tensor(inputs(arch, N), device="cuda")
    keep = x.clone()
    t.loss_and_grad(x, seed=SEED, iteration=PHASES["post"])
    assert torch.equal(x, keep)


def test_same_inputs_same_bits_and_rows_independent_of_the_batch():
    a = run("T16", 3, "post")
    a = dict(a, grads={k: v.clone() for k, v in a["grads"].items()})   # views of the buffer the next call writes
    b = run("T16", 3, "post")
    for k in tw.TERMS:
        assert a[k] == b[k], k
    for k in ("means", "log_var", "z", "recon"):
        assert torch.equal(a[k], b[k]), k
    for k, g in a["grads"].items():
        assert torch.equal(g, b["grads"][k]), k
    one, eight = run("T16", 1, "post"), run("T16", 8, "post")
    for k in ("means", "log_var", "z", "recon"):
        assert torch.equal(one[k][0], a[k][0]) and torch.equal(a[k], eight[k][:3]), k


@pytest.mark.parametrize("n, zero", [(1, False), (63, False), (1025, False), (63, True)])
def test_adam_flat_matches_torch_adam(n, zero):
    """5 steps on identical gradients against torch.optim.Adam in fp32 on the CPU: within 2 ulp of the parameter"""
    from sdfest_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(n)
    p0 = rng.uniform(-1, 1, n).astype(np.float32)
    grads = [np.zeros(n, np.float32) if zero else (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32)
             for _ in range(5)]
    ref = torch.tensor(p0.copy(), requires_grad=True)
    opt = torch.optim.Adam([ref], lr=1e-3)
    p = torch.tensor(p0, device="cuda")
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    for i, g in enumerate(grads):
        ref.grad = torch.tensor(g)
        opt.step()
        gd = torch.tensor(g, device="cuda")
        rc = L.sdfr_adam_flat(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(), n, 1e-3, 0, None)
        torch.cuda.synchronize()
        assert rc == 0 and int(step.item()) == i + 1
        r = ref.detach().numpy()
        ulps = np.abs(p.cpu().numpy().astype(np.float64) - r) / np.spacing(np.abs(r))
        assert ulps.max() <= 2.0, (i, ulps.max())
    if zero:
        assert np.array_equal(p.cpu().numpy(), p0)
    else:
        assert not np.array_equal(p.cpu().numpy(), p0)


def test_trajectory_across_the_phase_switch_matches_twin():
    """T16, two blobs volumes at 16^3, 30 steps with warm_up_iterations = 10: the total loss of every step against the
    float64 twin on the same schedule and eps.  Tolerance: torch fp32 on the CPU differs from the float64 twin by at most
    4.05e-7 relative per step on this run (measured with vae_train_twin.Twin(dtype=torch.float32)); 10 x that is allowed,
    4.05e-6 -- Adam's early steps amplify the sign noise of gradients near zero.  Observed on MI355X: 5.4e-7."""
    from sdfest_amd import SDFVAETrainer
    config = dict(tw.T16, warm_up_iterations=10)
    state = tw.random_state(config, 11)
    x = tw.blobs_at(16, (0, 1))
    twin = tw.Twin(config, state)
    t = SDFVAETrainer(config, state)
    xg = torch.tensor(x, device="cuda")
    got = torch.stack([t.step(xg, seed=100 + it) for it in range(30)]).cpu().numpy()
    ref = np.array([twin.step(x, et.normal_eps(100 + it, 2, 3))["total"] for it in range(30)])
    rel = np.abs(got[:, 5] - ref) / np.abs(ref)
    print(f"trajectory: worst per-step relative difference {rel.max():.2e} (step {int(rel.argmax()) + 1})")
    assert t.iteration == 30
    assert rel.max() <= 4.05e-6, rel
    assert got[29, 5] < got[10, 5]       # step 30 below step 11: an update that does nothing cannot pass
    assert got[9, 5] < got[0, 5]         # ... nor within the warm-up phase, where the loss is the same function


def test_state_dict_checkpoint_fit_and_command_line(tmp_path):
    from sdfest_amd import SDFVAE, SDFVAETrainer
    import yaml
    config = dict(tw.T16, warm_up_iterations=2, batch_size=2)
    x = torch.tensor(tw.blobs_at(16, (0, 1)), device="cuda")
    t = SDFVAETrainer(config, seed=3)
    for _ in range(2):
        t.step(x)
    # the trained state in the inference handles
    vae = SDFVAE.from_config(config, t.state_dict(), sdf_size=16)
    with torch.no_grad():
        z, means, log_var = vae.encode(x, seed=1)
        assert vae.decode(z).shape == (2, 1, 16, 16, 16) and torch.isfinite(means).all()
        assert torch.equal(t.vae().decode(z), vae.decode(z))
    assert list(t.state_dict()) == [k for k, _ in t._shapes]
    # a resumed run continues bit for bit (across the phase switch)
    path = str(tmp_path / "run.ckpt")
    t.save_checkpoint(path)
    u = SDFVAETrainer(config, seed=99)
    u.load_checkpoint(path)
    assert u.iteration == 2
    for _ in range(2):
        a, b = t.step(x), u.step(x)
        assert torch.equal(a, b)
    assert all(torch.equal(v, u.state_dict()[k]) for k, v in t.state_dict().items())
    assert torch.equal(t._exp_avg, u._exp_avg) and torch.equal(t._exp_avg_sq, u._exp_avg_sq)
    # fit on a folder of four volumes: two epochs of two batches
    folder = tmp_path / "volumes"
    folder.mkdir()
    for i, v in enumerate(tw.blobs_at(16, (0, 1, 2, 3))):
        np.save(str(folder / f"{i:05d}.npy"), v[0])
    f = SDFVAETrainer(config, seed=4)
    logged = []
    epochs = f.fit(str(folder), iterations=4, log_every=2, callback=lambda it, terms: logged.append((it, terms["total"])))
    assert epochs == 2 and f.iteration == 4 and [it for it, _ in logged] == [2, 4]
    assert all(np.isfinite(v) for _, v in logged)
    # the command line writes a .pt / .yaml pair that from_config loads
    cfg_path, out = str(tmp_path / "cfg.yaml"), str(tmp_path / "model")
    with open(cfg_path, "w") as fh:
        yaml.safe_dump(dict(config, iterations=3, pc_weight=0.0, dataset_path=str(folder)), fh)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_vae.py"), "--config", cfg_path, "--out", out,
                           "--seed", "4", "--log_every", "0"], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr
    with open(out + ".yaml") as fh:
        saved = yaml.safe_load(fh)
    assert saved["model"] == "./model.pt" and saved["latent_size"] == 3
    state = torch.load(out + ".pt", map_location="cpu")
    model = SDFVAE.from_config(saved, state, sdf_size=saved["sdf_size"])
    with torch.no_grad():
        assert torch.isfinite(model.decode(z)).all()
