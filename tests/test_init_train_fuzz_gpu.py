"""GPU: seeded random initialisation networks (tests/init_train_cases.py::draw -- 1 ... 4 backbone layers of 2 ... 140
columns on 1, 3, 4 or 6 input columns, repeated widths and a doubled last width so that residual links are taken, a first
layer as wide as the points now and then, BatchNorm, dense and residual flags at random, heads of 1 ... 3 layers up to
300 columns, latent sizes 1 ... 70, quaternion or 72 cells, 1 ... 6 sets of 1 ... 700 points) through the trainer
(sdfest_amd.SDFPoseNetTrainer over csrc/initnet_train.hip) against the float64 twin, with the bounds of
tests/test_init_train_edges_gpu.py, twice for the same bits.  A seed's case is the first sub-draw of weights, inputs and
BatchNorm-bias offset at which the comparison means something (tests/test_init_train_cases_cpu.py)."""
import pytest

import init_train_cases as ic
from test_init_train_edges_gpu import compare, compare_stats, new_trainer, run, same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", ic.default_seeds())
def test_random_architecture_matches_float64_twin(seed):
    """Observed on MI355X, the largest share of each bound over the 16 default seeds: gradients 0.27 (seed 8,
    _backbone._linear_layers.1.weight: 3.1e-5 of its maximum against a floor of 1.1e-5), loss terms 0.25 (seed 12,
    total), output rows 0.13, running statistics 0.11; null tensors at most 3.4e-6."""
    c = ic.case(seed)
    assert c is not None, f"seed {seed}: none of {ic.SUB_DRAWS} sub-draws meets the conditions"
    assert ic.accepted(ic.tabled(c)), ic.tabled(c)
    t = new_trainer(c)
    a = run(c, t)
    same_bits(a, run(c, t), c.name)
    compare(c, a)
    compare_stats(c)
