"""GPU: ``LMRefiner`` and ``SDFPipeline.refine`` end to end at the smallest sizes -- the mug decoder, a 64 x 48 camera,
targets rendered by the project's own forward at a known pose and latent, a start 5 mm, 3 degrees and 2 % of scale away
(the latent + 0.05 N(0, 1) where the shape is refined); and K = 2 objects from V = 2 cameras through
``estimate_objects`` on the scene of tests/test_multi_object_views_gpu.py.

Every iteration is held against the numpy twin (tests/lm_twin.py) fed the GPU's own Gram matrices at that iterate, with
the check of tests/test_lm_step_gpu.py."""
import numpy as np
import pytest
import torch

import _loop_scenes as S
import lm_twin as tw
from test_lm_step_gpu import check_against_twin
from test_multi_object_views_gpu import F, H, W, scene  # noqa: F401  (the module-scoped scene fixture)
from test_sdfpipeline_gpu import T, make_config, mug_weights, plausible_init_state

pytestmark = pytest.mark.gpu

CW, CH, CF, THR = 64, 48, 80.0, 0.005
D_POS, D_ANGLE, D_SCALE, D_LATENT = 0.005, np.radians(3.0), 0.02, 0.05     # the perturbation of the start


def small_scene(V, shape, seed=3):
    """dict(truth, start (1, 8 + L) float32 rows, target (V,CH,CW), cam_pos, cam_quat): the mug at 0.3 m seen by V cameras
    (the second one shifted and turned 20 degrees about y), rendered at the truth by ``render_depth_gpu``"""
    from sdfest_amd import Camera, render_depth_gpu
    dec, d = S.mug_decoder()
    cam = Camera(CW, CH, CF, CF, CW / 2, CH / 2, pixel_center=0.5)
    rng = np.random.default_rng(seed)
    a = np.deg2rad(20.0)
    cam_pos = np.array([[0.0, 0.0, 0.0], [0.3 * np.tan(a), 0.005, -0.01]])[:V]
    cam_quat = np.array([[0.0, 0.0, 0.0, 1.0], [0.0, np.sin(a / 2), 0.0, np.cos(a / 2)]])[:V]
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    z = d["z"][9] * 0.4
    truth = np.concatenate([[0.01, -0.005, -0.3], q, [0.05], z])
    images = []
    with torch.no_grad():
        sdf = dec.decode(T(z[None]))[0, 0]
        for v in range(V):
            qc = cam_quat[v] * np.array([-1, -1, -1, 1.0])
            images.append(render_depth_gpu(sdf, T(S._qrot(qc, truth[0:3] - cam_pos[v])), T(S._qmul(qc, q)),
                                           T(1.0 / truth[7]), None, None, None, THR, cam))
    target = torch.stack(images).contiguous()
    assert (target > 0).sum(dim=(1, 2)).min().item() >= 150
    axis, dp = rng.normal(size=3), rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    start = truth.copy()
    start[0:3] += D_POS * dp / np.linalg.norm(dp)
    start[3:7] = S._qmul(np.append(axis * np.sin(D_ANGLE / 2), np.cos(D_ANGLE / 2)), q)
    start[7] *= 1.0 + D_SCALE
    if shape:
        start[8:] += D_LATENT * rng.normal(size=z.size)
    return dict(dec=dec, cam=cam, truth=truth, start=T(start[None]), target=target, cam_pos=T(cam_pos),
                cam_quat=T(cam_quat), V=V)


def pipeline_from(sc, iterations=0, **extra):
    """an SDFPipeline whose initialisation is the scene's start and whose loop runs `iterations` Adam iterations"""
    from sdfest_amd import SDFPipeline
    cfg = make_config(CW, CH, CF, CF, CW / 2, CH / 2, THR, iterations, far_field=2.0, **extra)
    s = sc["start"]
    fixed = lambda *a: (s[:, 8:].clone(), s[:, 0:3].clone(), s[0, 7:8].clone(), s[:, 3:7].clone())
    pipe = SDFPipeline(cfg, vae_state_dict=mug_weights(), init_network=fixed)
    depth = sc["target"]
    args = (torch.ones_like(depth, dtype=torch.bool), torch.zeros(depth.shape + (3,), device="cuda"))
    return pipe, lambda shape: pipe(depth.clone(), *args, camera_positions=sc["cam_pos"],
                                    camera_orientations=sc["cam_quat"], shape_optimization=shape)


def pose_error(row, truth):
    """(metres, degrees, relative scale) between a row and the truth"""
    row, truth = np.asarray(row, np.float64), np.asarray(truth, np.float64)
    c = abs(np.dot(row[3:7] / np.linalg.norm(row[3:7]), truth[3:7] / np.linalg.norm(truth[3:7])))
    return (np.linalg.norm(row[0:3] - truth[0:3]), np.degrees(2 * np.arccos(min(1.0, c))), abs(row[7] / truth[7] - 1.0))


def iterate_against_twin(refiner, n, what):
    """n iterations of a started refiner, one by one: each step's decisions equal the twin's fed the GPU's own Gram
    matrices, and its new trial rows and solve meet tests/test_lm_step_gpu.py's check.  Returns the states (n, K, 16)."""
    K, V, Tn, Fn = refiner.K, refiner.V, refiner.T, refiner.F
    n_ = lambda t: t.detach().cpu().numpy()
    cq = n_(refiner.cam_quat)
    states = []
    for it in range(n):
        init = refiner._init
        refiner.evaluate()
        before = [n_(t) for t in (refiner.gram_trial, refiner.params_trial, refiner.params_cur, refiner.gram_cur,
                                  refiner.state)]
        if init:     # (the current buffers and the state hold anything before init)
            before[2:] = [np.zeros_like(a) for a in before[2:]]
        refiner.solve()
        refiner.iterations += 1
        want = tw.lm_step(before[0].reshape(K, V, Fn, Fn), before[1], before[2], before[3].reshape(K, V, Fn, Fn),
                          before[4], cq, Tn, init, latent_weight=refiner.latent_weight, min_overlap=refiner.min_overlap,
                          **refiner.constants)
        got = dict(trial=n_(refiner.params_trial), cur=n_(refiner.params_cur),
                   gram=n_(refiner.gram_cur).reshape(K, V, Fn, Fn), state=n_(refiner.state), step=n_(refiner.step))
        check_against_twin(got, want, want[5], Tn, (what, it))
        states.append(got["state"])
    return np.array(states)


def by_construction(states, min_overlap):
    """the accepted costs fall strictly, every accepted count keeps min_overlap of its predecessor, final <= initial"""
    for k in range(states.shape[1]):
        S_ = states[:, k]
        live = [0] + [i for i in range(1, len(S_)) if S_[i, tw.ACCEPTED] > S_[i - 1, tw.ACCEPTED]]
        costs, counts = S_[live, tw.COST], S_[live, tw.COUNT]
        assert np.all(np.diff(costs) < 0), costs
        assert np.all(counts[1:] >= min_overlap * counts[:-1]), counts
        assert S_[-1, tw.COST] <= S_[0, tw.COST_INIT] and S_[0, tw.COST] == S_[0, tw.COST_INIT]


@pytest.mark.parametrize("V, shape", [(1, False), (2, True)], ids=["K1-V1-pose", "K1-V2-shape"])
def test_refine_one_object(V, shape):
    from sdfest_amd import LMRefiner
    sc = small_scene(V, shape)
    pipe, run = pipeline_from(sc)
    with pytest.raises(RuntimeError, match="needs an estimate"):
        pipe.refine()
    out = run(shape)
    start = pipe._last_estimate.params[None].clone()
    assert torch.equal(start, sc["start"])                       # (no Adam iteration: the loop's rows are its start)
    assert torch.allclose(torch.cat([out[0], out[1], out[2][:, None], out[3]], dim=1), start, rtol=0, atol=1e-6)
    n = 6
    # by hand, step by step against the twin
    refiner = LMRefiner(pipe, 1, V, shape).start(start, sc["target"], sc["cam_pos"], sc["cam_quat"])
    states = iterate_against_twin(refiner, n + 1, f"V={V} shape={shape}")
    by_construction(states, 0.5)
    # the front door does the same launches: the same bits
    (position, orientation, scale, latent), report = pipe.refine(n)
    rows = refiner.params_cur
    assert torch.equal(pipe._last_estimate.params, rows[0])
    assert torch.equal(position, rows[:, 0:3]) and torch.equal(scale, rows[:, 7]) and torch.equal(latent, rows[:, 8:])
    assert torch.allclose(orientation, rows[:, 3:7], rtol=0, atol=1e-6)
    assert report.accepted.tolist() == [int(states[-1, 0, tw.ACCEPTED])] and report.accepted[0] >= 1
    assert float(report.final_cost[0]) < float(report.initial_cost[0]) == states[0, 0, tw.COST_INIT]
    assert float(report.final_count[0]) >= 150 and report.status.shape == (1,) and report.final_lambda.shape == (1,)
    assert abs(float(orientation.norm()) - 1.0) <= 1e-6
    e0, e1 = pose_error(sc["start"][0].cpu().numpy(), sc["truth"]), pose_error(rows[0].cpu().numpy(), sc["truth"])
    print(f"V={V} shape={shape}: Phi {float(report.initial_cost[0]):.3e} -> {float(report.final_cost[0]):.3e}, accepted "
          f"{int(report.accepted[0])} rejected {int(report.rejected[0])} status {int(report.status[0])}; pose error "
          f"{e0[0] * 1e3:.2f} mm {e0[1]:.2f} deg {e0[2] * 100:.2f} % -> {e1[0] * 1e3:.2f} mm {e1[1]:.2f} deg {e1[2] * 100:.2f} %")
    if shape:
        assert not torch.equal(latent, sc["start"][:, 8:])
        pipe.refine(2, shape_optimization=False)
        assert torch.equal(pipe._last_estimate.params[8:], latent[0])       # T = 0: the latent is not touched
    else:
        assert torch.equal(latent, sc["start"][:, 8:])                      # bit for bit the start's
        # write-back: the uncertainty is evaluated at the refined rows (camera at the origin: world = camera frame)
        v = pipe._uncertainty_views()
        assert torch.allclose(v["position"][0], position[0], rtol=0, atol=1e-7)
        assert torch.allclose(v["inv_scale"][0], 1.0 / scale[0], rtol=1e-6, atol=0)
        assert pipe.pose_uncertainty().information.shape == (1, 7, 7)


def test_refine_after_estimate_objects(scene):  # noqa: F811
    from sdfest_amd import LMRefiner, SDFPipeline
    K, V = 2, 2
    frames, masks = scene["frames"], scene["masks"][:K].contiguous()
    cfg = make_config(W, H, F, F, W / 2, H / 2, 0.005, 4, far_field=2.0)
    pipe = SDFPipeline(cfg, vae_state_dict=mug_weights(), init_state_dict=plausible_init_state())
    out = pipe.estimate_objects(frames, masks, scene["cam_pos"], scene["cam_quat"], shape_optimization=False)
    loop = pipe._last_estimate
    start = loop.params.clone()
    refiner = LMRefiner(pipe, K, V, False).start(start, loop.target, loop.cam_pos, loop.cam_quat)
    states = iterate_against_twin(refiner, 4, "estimate_objects")
    by_construction(states, 0.5)
    (position, orientation, scale, latent), report = pipe.refine(3)          # shape_optimization=None: as the call, off
    assert position.shape == (K, 3) and orientation.shape == (K, 4) and scale.shape == (K,) and latent.shape == out[3].shape
    assert torch.equal(loop.params, refiner.params_cur) and torch.equal(latent, out[3])
    assert torch.equal(position, refiner.params_cur[:, :3]) and torch.equal(scale, refiner.params_cur[:, 7])
    assert (orientation.norm(dim=1) - 1.0).abs().max().item() <= 1e-6
    assert (report.final_cost <= report.initial_cost).all() and report.status.shape == (K,)
    print("estimate_objects + refine(3): Phi", report.initial_cost.tolist(), "->", report.final_cost.tolist(), "accepted",
          report.accepted.tolist(), "rejected", report.rejected.tolist(), "status", report.status.tolist())
    # the refined rows are what the uncertainty now looks at
    assert torch.equal(pipe._uncertainty_views()["latent"], latent)
    assert pipe.pose_uncertainty().information.shape == (K, 7, 7)


def test_fixed_point_stays_put():
    """the truth as the start, a noise-free target: the gradient is rounding noise at most (the target's camera-frame
    poses were formed on the host, the refiner's by its kernel; where both round alike the residual is exactly zero and
    the row converges at once) and the estimate must stay two orders below the perturbation the other tests start from"""
    from sdfest_amd import LMRefiner
    sc = small_scene(2, False)
    truth = T(sc["truth"][None])
    refiner = LMRefiner((sc["dec"], sc["cam"], THR), 1, 2, False).start(truth, sc["target"], sc["cam_pos"], sc["cam_quat"])
    refiner.iterate(5)
    e = pose_error(refiner.params_cur[0].cpu().numpy(), sc["truth"])
    factors = (e[0] / D_POS, np.radians(e[1]) / D_ANGLE, e[2] / D_SCALE)
    rep = refiner.report()
    print(f"fixed point: moved by {factors[0]:.2e} / {factors[1]:.2e} / {factors[2]:.2e} of the perturbation "
          f"(position / angle / scale), Phi {float(rep.initial_cost[0]):.3e} -> {float(rep.final_cost[0]):.3e}, "
          f"accepted {int(rep.accepted[0])}, status {int(rep.status[0])}")
    assert max(factors) < 1e-2
    assert torch.isfinite(refiner.params_cur).all() and float(rep.final_cost[0]) <= float(rep.initial_cost[0])


def test_config_key_gauss_newton_iterations():
    """0 (or no key): bit for bit the pipeline's estimate; n > 0: what ``refine(n)`` returns"""
    sc = small_scene(1, False)
    n = 6
    plain, keyed0, keyed = (pipeline_from(sc, 2, **extra) for extra in ({}, {"gauss_newton_iterations": 0},
                                                                        {"gauss_newton_iterations": n}))
    a, b, c = plain[1](False), keyed0[1](False), keyed[1](False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    refined, report = plain[0].refine(n)
    for x, y in zip(refined, c):
        assert x.shape == y.shape and torch.equal(x, y)
    # n trials were judged (or the row froze before)
    assert int(report.accepted[0]) + int(report.rejected[0]) == n or int(report.status[0]) != 0
    assert float(report.final_cost[0]) <= float(report.initial_cost[0])


def test_config_key_with_hypotheses_and_frames():
    """the key behind ``estimate_hypotheses`` (all N rows are refined, the winner the loop selected is returned from the
    refined rows) and ``estimate_frames``: what the plain call followed by ``refine`` gives, bit for bit"""
    from test_hypotheses_gpu import Q_TRUE, mug_scene, small_pipeline
    n = 3
    plain, keyed = small_pipeline(), small_pipeline(gauss_newton_iterations=n)
    depth, mask, _ = mug_scene(plain, Q_TRUE)
    a = plain.estimate_hypotheses(depth, mask, hypotheses=3, shape_optimization=False)
    c = keyed.estimate_hypotheses(depth, mask, hypotheses=3, shape_optimization=False)
    winner = plain.last_hypotheses()["winner"]
    (position, orientation, scale, latent), report = plain.refine(n)
    assert position.shape == (3, 3) and report.status.shape == (3,) and keyed.last_hypotheses()["winner"] == winner
    rows = plain._last_estimate.params[winner]
    assert [tuple(t.shape) for t in c] == [tuple(t.shape) for t in a] == [(1, 3), (1, 4), (1,), (1, 8)]
    assert torch.equal(c[0][0], rows[0:3]) and torch.equal(c[1][0], rows[3:7]) and torch.equal(c[2][0], rows[7])
    assert torch.equal(c[3][0], rows[8:]) and (report.final_cost <= report.initial_cost).all()
    # K frames with one object each
    frames, masks = torch.stack([depth, depth]).contiguous(), torch.stack([mask, mask]).contiguous()
    plain.estimate_frames(frames.clone(), masks, shape_optimization=False)
    refined, _ = plain.refine(n)
    got = keyed.estimate_frames(frames.clone(), masks, shape_optimization=False)
    for x, y in zip(refined, got):
        assert x.shape == y.shape and torch.equal(x, y)
