"""GPU: ``LMRefiner(pc_weight=)`` and ``SDFPipeline.refine(pc_weight=)`` on the scenes of tests/test_refine_gpu.py -- the
point-cloud term of the loop's objective inside the Levenberg-Marquardt refinement.

At every iteration the matrices handed to ``sdfr_lm_step`` are bit for bit the twin's combination
(tests/pc_information_twin.py) of the refiner's own depth and point-cloud Gram matrices, and the step's decisions are the
numpy LM twin's on them (``test_refine_gpu.iterate_against_twin``)."""
import numpy as np
import pytest
import torch

import lm_twin as ltw
import pc_information_twin as ptw
from test_refine_gpu import (D_ANGLE, D_POS, D_SCALE, THR, by_construction, iterate_against_twin, pipeline_from, pose_error,
                             small_scene)
from test_sdfpipeline_gpu import T

pytestmark = pytest.mark.gpu


def check_every_evaluation(refiner):
    """wraps ``refiner.evaluate``: after each one the combined matrices are the twin's bits and the point-cloud term's
    counts are the target's pixels"""
    plain = refiner.evaluate
    F = refiner.F

    def evaluate(st=None):
        plain(st)
        pixels = (refiner.target > 0).sum(dim=(1, 2)).to(torch.float64)
        gd, gp = refiner.gram_depth_trial.cpu().numpy(), refiner.gram_pc_trial.cpu().numpy()
        want = ptw.combine(gd, gp, refiner.K, refiner.V, refiner.T, refiner.pc_weight)
        assert np.array_equal(refiner.gram_trial.cpu().numpy(), want, equal_nan=True)
        assert torch.equal(refiner.gram_pc_trial[:, F - 1, F - 1], pixels) and pixels.min().item() >= 150
        assert torch.equal(refiner.gram_pc_trial, refiner.gram_pc_trial.transpose(1, 2))
        assert (refiner.gram_pc_trial[:, F - 2, F - 2] > 0).all()      # the residuals are not all zero

    refiner.evaluate = evaluate
    return refiner


@pytest.mark.parametrize("V, shape", [(1, False), (2, True)], ids=["K1-V1-pose", "K1-V2-shape"])
def test_refine_with_the_point_cloud_term(V, shape):
    from sdfest_amd import LMRefiner
    sc = small_scene(V, shape)
    pipe, run = pipeline_from(sc)
    run(shape)
    start = pipe._last_estimate.params[None].clone()
    n = 6
    refiner = check_every_evaluation(LMRefiner(pipe, 1, V, shape, pc_weight=1.0))
    refiner.start(start, sc["target"], sc["cam_pos"], sc["cam_quat"])
    states = iterate_against_twin(refiner, n + 1, f"pc V={V} shape={shape}")
    by_construction(states, 0.5)
    # the front door does the same launches: the same bits
    (position, orientation, scale, latent), report = pipe.refine(n, pc_weight=1.0)
    rows = refiner.params_cur
    assert torch.equal(pipe._last_estimate.params, rows[0])
    assert torch.equal(position, rows[:, 0:3]) and torch.equal(scale, rows[:, 7]) and torch.equal(latent, rows[:, 8:])
    assert float(report.final_cost[0]) <= float(report.initial_cost[0]) == states[0, 0, ltw.COST_INIT]
    # Phi is the combined one: above the depth term's at the same start
    plain = LMRefiner(pipe, 1, V, shape).start(start, sc["target"], sc["cam_pos"], sc["cam_quat"]).iterate(1).report()
    assert float(report.initial_cost[0]) > float(plain.initial_cost[0]) > 0
    e0, e1 = pose_error(sc["start"][0].cpu().numpy(), sc["truth"]), pose_error(rows[0].cpu().numpy(), sc["truth"])
    print(f"pc V={V} shape={shape}: Phi {float(report.initial_cost[0]):.3e} -> {float(report.final_cost[0]):.3e}, accepted "
          f"{int(report.accepted[0])} rejected {int(report.rejected[0])} status {int(report.status[0])}; pose error "
          f"{e0[0] * 1e3:.2f} mm {e0[1]:.2f} deg {e0[2] * 100:.2f} % -> {e1[0] * 1e3:.2f} mm {e1[1]:.2f} deg {e1[2] * 100:.2f} %")
    # the config key is the keyword
    keyed, run_keyed = pipeline_from(sc, gauss_newton_pc_weight=1.0)
    run_keyed(shape)
    (p2, o2, s2, z2), _ = keyed.refine(n)
    assert torch.equal(p2, position) and torch.equal(o2, orientation) and torch.equal(s2, scale) and torch.equal(z2, latent)


@pytest.mark.parametrize("V, shape", [(1, False), (2, True)], ids=["K1-V1-pose", "K1-V2-shape"])
def test_truth_start_stays_put_with_the_point_cloud_term(V, shape):
    """the truth as the start, a noise-free target: after every iteration the estimate is within tests/test_refine_gpu.py's
    bound for its own truth start -- a hundredth of the perturbation the other tests start from"""
    from sdfest_amd import LMRefiner
    sc = small_scene(V, shape)
    truth = T(sc["truth"][None])
    refiner = LMRefiner((sc["dec"], sc["cam"], THR), 1, V, shape, pc_weight=1.0).start(truth, sc["target"], sc["cam_pos"],
                                                                                      sc["cam_quat"])
    worst = []
    for it in range(5):
        refiner.iterate(1)
        e = pose_error(refiner.params_cur[0].cpu().numpy(), sc["truth"])
        worst.append((e[0] / D_POS, np.radians(e[1]) / D_ANGLE, e[2] / D_SCALE))
    rep = refiner.report()
    print(f"pc truth start V={V} shape={shape}: moved by at most {np.max(worst, axis=0)} of the perturbation (position / "
          f"angle / scale), Phi {float(rep.initial_cost[0]):.3e} -> {float(rep.final_cost[0]):.3e}, accepted "
          f"{int(rep.accepted[0])}, status {int(rep.status[0])}")
    assert torch.isfinite(refiner.params_cur).all() and float(rep.final_cost[0]) <= float(rep.initial_cost[0])
    assert np.max(worst) < 1e-2


def test_zero_weight_is_the_refiner_without_the_argument():
    from sdfest_amd import LMRefiner
    sc = small_scene(2, True)
    parts = (sc["dec"], sc["cam"], THR)
    a = LMRefiner(parts, 1, 2, True).start(sc["start"], sc["target"], sc["cam_pos"], sc["cam_quat"]).iterate(4)
    b = LMRefiner(parts, 1, 2, True, pc_weight=0.0).start(sc["start"], sc["target"], sc["cam_pos"], sc["cam_quat"]).iterate(4)
    assert torch.equal(a.params_cur, b.params_cur) and torch.equal(a.state, b.state) and torch.equal(a.gram_cur, b.gram_cur)
    assert b.gram_pc_trial is None and b.gram_depth_trial is None and not hasattr(b, "points")
    with pytest.raises(ValueError, match="pc_weight"):
        LMRefiner(parts, 1, 2, True, pc_weight=-1.0)


def test_refine_without_the_key_is_the_explicit_zero():
    sc = small_scene(1, False)
    n = 4
    (plain, run_plain), (zero, run_zero) = pipeline_from(sc), pipeline_from(sc)
    run_plain(False), run_zero(False)
    a, ra = plain.refine(n)
    b, rb = zero.refine(n, pc_weight=0.0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(plain._last_refiner.state, zero._last_refiner.state)
    assert plain._last_refiner.gram_pc_trial is None
    # on and off are two refiners of one pipeline; off again gives the first bits again
    run_plain(False)
    c, _ = plain.refine(n, pc_weight=1.0)
    assert plain._last_refiner.gram_pc_trial is not None and not torch.equal(c[0], a[0])
    run_plain(False)
    d, _ = plain.refine(n)
    for x, y in zip(a, d):
        assert torch.equal(x, y)
