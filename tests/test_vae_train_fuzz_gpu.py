"""GPU: seeded random VAE architectures (tests/vae_train_cases.py::draw -- volumes 8 ... 20, latent sizes 1 ... 8,
batches 1 ... 5, 0 ... 3 encoder convolutions with kernels 1 ... 5, strides 1 ... 3, padding 0 ... 2 and up to 40 channels,
pools with k <= 3 and strides 1 ... 3, 0 ... 2 encoder Linears, 0 ... 2 hidden decoder Linears, 1 ... 3 decoder convolutions
behind resizes up and down, now and then a ReLU'd last layer, tsdf False / 0.1 / 0.3) through the trainer
(sdfest_amd.SDFVAETrainer over csrc/vae_train.hip) in both phases against the float64 twin, twice for the same bits, and
at N = 1 for rows that do not depend on the batch.  A seed's case is its first sub-draw at which the comparison means
something (no dead gradient, no value within 1e-5 of a branch, torch fp32 on the CPU within 1e-5:
tests/test_vae_train_cases_cpu.py)."""
import os

import pytest
import torch

import vae_train_cases as vc
from test_vae_train_edges_gpu import compare, run, same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(int(os.environ.get("SDFR_FUZZ_SEEDS", "16"))))
def test_random_architecture_matches_float64_twin(seed):
    """Bounds: those of test_gradients_and_loss_terms_match_float64_twin (every gradient element within 1e-4 of its
    tensor's float64 maximum; loss terms and forward arrays 1e-5 + 1e-5).  Observed on MI355X over the 16 default seeds:
    the worst gradient element 9.9e-6 of its tensor's maximum (seed 12, warm, encoder.linear_means.weight, behind a
    Linear 891 -> 1 on which torch fp32 on the CPU is 1.0e-5 from float64; next 5.3e-6, seed 6), the loss terms at most
    0.307 (seed 2, post) and the forward arrays 0.158 of their bound."""
    from sdfest_amd import SDFVAETrainer
    c = vc.case(seed)
    assert c is not None, f"seed {seed}: none of {vc.SUB_DRAWS} sub-draws meets the conditions"
    what = f"seed {seed}, sub-draw {c.sub}: {vc.describe(c.config)}"
    print(what)
    t = SDFVAETrainer(c.config, c.state)
    for phase in vc.PHASES:
        a = run(t, c, phase)
        same_bits(a, run(t, c, phase), f"{what}, {phase}")
        compare(c, phase, a)
        one = run(t, c, phase, rows=1)
        for k in ("means", "log_var", "z", "recon"):
            assert torch.equal(one[k][0], a[k][0]), f"{what}, {phase}: row 0 of {k} depends on the batch"
