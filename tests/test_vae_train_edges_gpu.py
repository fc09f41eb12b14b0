"""GPU: the VAE trainer (sdfest_amd.SDFVAETrainer over csrc/vae_train.hip) on the hand-written edge architectures of
tests/vae_train_cases.py, in both phases, against the float64 twin (tests/vae_train_twin.py) -- the comparison of
test_vae_train_gpu.py::test_gradients_and_loss_terms_match_float64_twin with the forward arrays added, at the shapes its
three architectures never reach: pools with overlapping and gapped windows, strided convolutions with padding and even
kernels, the weight gradient's tiles on every side of their sizes, resizes down and from one voxel, both linear data
gradients at their switch, and the op lists the backward special-cases.  tests/test_vae_train_cases_cpu.py asserts that
the edges take each of those paths and that no branch or dead gradient makes a case vacuous."""
import functools

import numpy as np
import pytest
import torch

import vae_train_cases as vc
import vae_train_twin as tw
from test_vae_train_gpu import close

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def trainer(name):
    from sdfest_amd import SDFVAETrainer
    c = vc.edge(name)
    return SDFVAETrainer(c.config, c.state)


def run(t, c, phase, rows=None):
    """loss_and_grad with the gradients cloned: they are views of the buffer the next call writes"""
    x = torch.tensor(c.x[:rows], device="cuda")
    out = t.loss_and_grad(x, seed=c.seed, iteration=vc.PHASES[phase])
    return dict(out, grads={k: v.clone() for k, v in out["grads"].items()})


def compare(c, phase, out):
    """every element of every parameter's gradient within 1e-4 of the tensor's float64 maximum, the same gradient set and
    shapes; the loss terms, means, log_var, z and recon within 1e-5 relative + 1e-5 absolute; z bitwise eps sd + means.
    Returns the worst gradient share and prints it with its tensor."""
    what = f"{c.name}, sub-draw {c.sub}, {phase}: {vc.describe(c.config)}"
    terms, grads, arrays = c.reference[phase]
    assert sorted(out["grads"]) == sorted(grads), what
    worst, where = 0.0, None
    for name, g64 in grads.items():
        g = out["grads"][name].cpu().numpy().astype(np.float64)
        assert g.shape == g64.shape, f"{what}: {name}"
        err = np.abs(g - g64).max() / np.abs(g64).max()      # the cases have no gradient that is identically zero
        if not err <= worst:
            worst, where = err, name
    print(f"{c.name} {phase}: worst gradient error {worst:.2e} of the tensor's maximum ({where})")
    try:
        used = max(close(out[k], terms[k]) for k in tw.TERMS)
        print(f"{c.name} {phase}: loss terms use {used:.3f} of the 1e-5 + 1e-5 bound")
        used = max(close(out[k].cpu(), ref) for k, ref in zip(("means", "log_var", "z", "recon"), arrays))
        print(f"{c.name} {phase}: means, log_var, z, recon use {used:.3f} of the 1e-5 + 1e-5 bound")
    except AssertionError as e:
        raise AssertionError(f"{what}: {e} of the 1e-5 + 1e-5 bound") from e
    eps = torch.tensor(c.eps, device="cuda")
    assert torch.equal(out["z"], eps * torch.exp(0.5 * out["log_var"]) + out["means"]), what
    assert worst <= 1e-4, f"{what}: {where}: {worst:.2e} of its maximum"
    return worst


def same_bits(a, b, what):
    for k in tw.TERMS:
        assert a[k] == b[k], f"{what}: {k}"
    for k in ("means", "log_var", "z", "recon"):
        assert torch.equal(a[k], b[k]), f"{what}: {k}"
    for k, g in a["grads"].items():
        assert torch.equal(g, b["grads"][k]), f"{what}: {k}"


@pytest.mark.parametrize("phase", list(vc.PHASES))
@pytest.mark.parametrize("name", list(vc.EDGES))
def test_edge_architecture_matches_float64_twin(name, phase):
    """Bounds: those of test_gradients_and_loss_terms_match_float64_twin.  torch fp32 on the CPU stays within 1e-5 of each
    tensor's maximum on every edge (3.2e-6 at most) and no value is within 1e-5 of a branch (test_vae_train_cases_cpu.py),
    so 1e-4 is at least ten times what fp32 in another order of summation costs and no flipped branch can explain an
    excess.  The gapped pool (k = 2, s = 3: a third of its input is read by no window) also runs twice for the same
    bits.  Observed on MI355X: the worst gradient element 1.4e-6 of its tensor's maximum (conv_k4_s2_p1, warm,
    encoder.linear_log_var.weight), the loss terms at most 0.051 and the forward arrays 0.182 (wgrad_wide) of their bound
    (DESIGN.md 3.14)."""
    c = vc.edge(name)
    assert vc.accepted(c.report), c.report
    out = run(trainer(name), c, phase)
    compare(c, phase, out)
    if name == "pool_gapped":
        same_bits(out, run(trainer(name), c, phase), f"{name} {phase}")
