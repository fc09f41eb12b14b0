#!/usr/bin/env python3
"""What the point-cloud term of the Gauss-Newton information costs and what it changes (the method of tools/bench_lm.py:
warmed up, samples INTERLEAVED over `--repeats` rounds, a sample being `--calls` consecutive calls).

Part 1, kernel: ``sdfr_pc_information`` on the C5 target's points in `--views` views (the same ~15 k points and the
start pose in every view, one shared volume) at T = 0 beside ``sdfr_pc_loss_backward`` on the same points (upstream
gradient = the residual), and at T = 8 beside ``sdfr_render_information_shape`` on the same views (the C5 render at the
start pose against the C5 target).  Device events.
Part 2, one ``LMRefiner`` iteration with ``pc_weight`` 0 and 1 on the C5 scene at 640x480, pose only and with shape,
K = 1 and K = 32.  Host clock around calls that end in a device synchronise.
Part 3, convergence: tools/bench_lm.py's schedules (50 Adam + 0 / 5 LM, 10 Adam + 10 LM) from the perturbed C5 start and
from G7 run C's start, with ``pc_weight`` 0 and 1: Phi and its two parts (mean squared depth residual, mean squared
point-cloud residual) before and after, accepted / rejected trials, the damping behind every accepted trial, the pose
error against the scene's truth (C5).
Part 4, the model against the objective at the C5 start: central finite differences of the depth part, the point-cloud
part and the combined Phi (``pc_weight`` = 1) along the seven pose tangent directions beside the model's slope 2 g.
Everything goes to profiles/bench_pc_information.json as found (a run of some `--parts` replaces those parts of an
existing file); none of it is a test gate."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from bench_information import event_sample, host_sample  # noqa: E402
from bench_lm import pose_error  # noqa: E402
from bench_shape_information import interleaved, report  # noqa: E402


def kernel_part(a):
    from _loop_scene import c5_scene
    from sdfest_amd import losses, pc_information, render_information
    from sdfest_amd.differentiable_renderer import forward_raw
    from sdfest_amd.generated_views import depth_to_pointsets
    sc = c5_scene(views=1)
    cam, init, B, T = sc["camera"], sc["init"], a.views, 8
    dev = sc["targets"].device
    sdf = sc["decoder"].decode(init[3])[0, 0].contiguous()
    pts1, counts = depth_to_pointsets(sc["targets"][:1], cam, tiled=True)
    M = int(counts[0])
    pts = pts1.repeat(B, 1).contiguous()
    offsets = (torch.arange(B + 1, device=dev) * M).to(torch.int32)
    pos, quat, scale = (t.repeat(B, *([1] * (t.dim() - 1))).contiguous() for t in (init[0], init[1], init[2]))
    isc = (1.0 / scale).contiguous()
    jac = torch.tensor(np.random.default_rng(1).normal(size=(64 ** 3, T)).astype(np.float32), device=dev)
    fx, fy, cx, cy, _ = cam.get_pinhole_camera_parameters(0.5)
    depth = forward_raw(sdf, pos, quat, isc, cam.width, cam.height, cx, cy, fx, fy, sc["config"]["threshold"])
    target = sc["targets"][:1].repeat(B, 1, 1).contiguous()
    r = losses._forward_raw(pts, offsets, M, pos, quat, scale, sdf)
    cases = {"pc_information_t0": lambda: pc_information(pts, offsets, sdf, pos, quat, scale, max_view_points=M),
             "pc_loss_backward": lambda: losses._backward_raw(r, pts, offsets, M, pos, quat, scale, sdf),
             "pc_information_t8": lambda: pc_information(pts, offsets, sdf, pos, quat, scale, jacobian=jac, tangents=T,
                                                         max_view_points=M),
             "render_information_shape_t8": lambda: render_information(depth, target, sdf, pos, quat, isc, cam,
                                                                       jacobian=jac, tangents=T)}
    g0, g8 = cases["pc_information_t0"](), cases["pc_information_t8"]()
    pick = list(range(8)) + [8 + T, 9 + T]
    agree = (g8[:, pick][:, :, pick] - g0).abs().max().item() / g0.abs().max().item()
    gs = cases["render_information_shape_t8"]()
    times = interleaved(cases, event_sample, a.calls, a.repeats)
    out = report(times, "us")
    med = lambda k: float(np.median(times[k]))
    out["pc_information_t0_over_pc_loss_backward"] = med("pc_information_t0") / med("pc_loss_backward")
    out["pc_information_t8_over_render_information_shape_t8"] = med("pc_information_t8") / med("render_information_shape_t8")
    out["pc_information_t8_over_t0"] = med("pc_information_t8") / med("pc_information_t0")
    out["views"], out["points_per_view"] = B, M
    out["included_pixels_per_view_of_the_depth_call"] = float(gs[0, 9 + T, 9 + T].item())
    out["max_abs_pose_block_t8_minus_t0_over_max"] = agree
    print(json.dumps({k: v for k, v in out.items() if not isinstance(v, dict)}), flush=True)
    return out


def iteration_part(a):
    from _loop_scene import c5_scene
    from sdfest_amd import LMRefiner
    sc = c5_scene(views=1)
    dec, cam, cfg, init = sc["decoder"], sc["camera"], sc["config"], sc["init"]
    row = torch.cat([init[0], init[1], init[2][:, None], init[3]], dim=1)
    out = {}
    for K in (1, 32):
        cases = {}
        target = sc["targets"][:1].repeat(K, 1, 1).contiguous()
        for shape in (False, True):
            for w in (0.0, 1.0):
                r = LMRefiner((dec, cam, cfg["threshold"]), K, 1, shape, pc_weight=w).start(row.repeat(K, 1), target)
                r.iterate(2)
                cases[f"K{K}_lm_iteration_{'shape' if shape else 'pose'}_pc{int(w)}"] = lambda r=r: r.iterate(1)
        times = interleaved(cases, host_sample, max(1, a.calls // 4), a.repeats)
        out.update(report(times, "us"))
        for s in ("pose", "shape"):
            k = f"K{K}_lm_iteration_{s}"
            out[f"K{K}_pc1_over_pc0_{s}"] = out[k + "_pc1"]["median_us"] / out[k + "_pc0"]["median_us"]
            print(f"K={K} {s}: iteration with the point-cloud term / without = {out[f'K{K}_pc1_over_pc0_{s}']:.2f}", flush=True)
    return out


def _parts_of(meter, rows):
    """(depth part, point-cloud part, depth count) of Phi at `rows` through a refiner built with pc_weight = 1"""
    from sdfest_amd.differentiable_renderer import _stream
    meter.params_trial.copy_(rows)
    meter._poses(_stream(meter.dev))
    meter.evaluate()
    F = meter.F
    gd, gp = meter.gram_depth_trial, meter.gram_pc_trial
    cd, cp = gd[:, F - 1, F - 1].sum(), gp[:, F - 1, F - 1].sum()
    return float(gd[:, F - 2, F - 2].sum() / cd), float(gp[:, F - 2, F - 2].sum() / cp), float(cd)


def convergence_part(a):
    from _loop_scene import c5_scene
    from bench_hypotheses import pipeline
    from sdfest_amd import LMRefiner, lm
    out = {}

    def schedule(make, run, truth, name):
        for adam, lm_n in ((50, 0), (50, 5), (10, 10)):
            for w in (0.0, 1.0):
                pipe = make(adam)
                run(pipe)
                loop, K, params = pipe._last_rows()
                shape, V = bool(loop.shape_opt), int(loop.V)
                meter = LMRefiner(pipe, K, V, shape, pc_weight=1.0).start(params, loop.target, loop.cam_pos, loop.cam_quat)
                before = _parts_of(meter, params)
                r = LMRefiner(pipe, K, V, shape, pc_weight=w).start(params, loop.target, loop.cam_pos, loop.cam_quat)
                lam_prev, accepted_lambdas = None, []
                for it in range(lm_n + 1):
                    r.iterate(1)
                    s = r.state.cpu()[0]
                    if it > 0 and s[lm.STATE["last_accept"]] == 1.0:
                        accepted_lambdas.append(lam_prev)
                    lam_prev = float(s[lm.STATE["lambda"]])
                rep = r.report()
                after = _parts_of(meter, r.params_cur)
                rec = {"pc_weight": w, "phi_after_adam": float(rep.initial_cost[0]), "phi_final": float(rep.final_cost[0]),
                       "depth_part_before_after": [before[0], after[0]], "pc_part_before_after": [before[1], after[1]],
                       "depth_count_before_after": [before[2], after[2]], "accepted": int(rep.accepted[0]),
                       "rejected": int(rep.rejected[0]), "status": int(rep.status[0]),
                       "lambda_of_accepted_trials": accepted_lambdas, "final_lambda": float(rep.final_lambda[0])}
                if truth is not None:
                    rec["pose_error_after_adam"] = pose_error(params[0].cpu().numpy(), truth)
                    rec["pose_error"] = pose_error(r.params_cur[0].cpu().numpy(), truth)
                out[f"{name}_adam{adam}_lm{lm_n}_pc{int(w)}"] = rec
                print(name, adam, lm_n, json.dumps(rec), flush=True)

    sc = c5_scene(views=1)
    init = sc["init"]
    q_true = np.array([0.2, 0.6, -0.15, 0.75])
    truth = np.concatenate([sc["p_true"][0].cpu().numpy(), q_true / np.linalg.norm(q_true), [0.055]])
    image = sc["targets"][0]
    mask = image > 0

    def make_c5(adam):
        pipe = pipeline(adam)
        pipe._nn_init_override = lambda *args: (init[3].clone(), init[0].clone(), init[2].clone(), init[1].clone())
        return pipe

    schedule(make_c5, lambda pipe: pipe(image.clone(), mask, torch.zeros((480, 640, 3), device=image.device)), truth, "c5")

    g7 = np.load(os.path.join(ROOT, "tests", "golden", "loop_g7.npz"))
    t = lambda x: torch.tensor(np.asarray(x, dtype=np.float32), device="cuda")
    g_init = g7["c_init"]

    def make_g7(adam):
        pipe = pipeline(adam)
        cfg = dict(pipe.config, threshold=float(g7["thr"]), far_field=50.0,
                   camera={"width": int(g7["c_W"]), "height": int(g7["c_H"]), "fx": float(g7["c_fx"]), "fy": float(g7["c_fy"]),
                           "cx": float(g7["c_cx"]), "cy": float(g7["c_cy"]), "pixel_center": 0.5})
        from sdfest_amd import SDFPipeline
        w = np.load(os.path.join(ROOT, "tests", "golden", "mug_decoder_weights.npz"))
        return SDFPipeline(cfg, vae_state_dict={k: w[k] for k in w.files},
                           init_network=lambda *args: (t(g_init[None, 8:]), t(g_init[None, 0:3]), t(g_init[7:8]),
                                                       t(g_init[None, 3:7])))

    depth = t(g7["c_depth_images"])
    schedule(make_g7, lambda pipe: pipe(depth.clone(), torch.ones_like(depth, dtype=torch.bool),
                                        torch.zeros(depth.shape + (3,), device="cuda"),
                                        camera_positions=t(g7["c_cam_pos"]), camera_orientations=t(g7["c_cam_quat"])),
             None, "g7c")
    return out


def gradient_part(a):
    from _loop_scene import c5_scene
    from sdfest_amd import LMRefiner, tangent_map
    from sdfest_amd.differentiable_renderer import _stream
    from sdfest_amd.pipeline import quaternion_multiply
    sc = c5_scene(views=1)
    init = sc["init"]
    row = torch.cat([init[0], init[1], init[2][:, None], init[3]], dim=1)
    r = LMRefiner((sc["decoder"], sc["camera"], sc["config"]["threshold"]), 1, 1, False, pc_weight=1.0).start(
        row, sc["targets"][:1])
    terms = {"depth": lambda: r.gram_depth_trial[0], "pc": lambda: r.gram_pc_trial[0], "combined": lambda: r.gram_trial[0]}

    def phi(rows):
        r.params_trial.copy_(rows)
        r._poses(_stream(r.dev))
        r.evaluate()
        return {k: (float(G()[8, 8] / G()[9, 9]), float(G()[9, 9]), G().clone()) for k, G in terms.items()}

    def moved(i, eps):     # the retraction of a step eps along tangent direction i
        out = row.clone().double()
        if i < 3:
            out[0, i] += eps
        elif i < 6:
            dq = torch.zeros(4, dtype=torch.float64, device=out.device)
            dq[i - 3], dq[3] = np.sin(eps / 2), np.cos(eps / 2)
            out[0, 3:7] = quaternion_multiply(dq[None], out[:, 3:7] / out[:, 3:7].norm())[0]
        else:
            out[0, 7] *= np.exp(eps)
        return out.float()

    at = phi(row)
    M = tangent_map(r.quat_c, r.inv_scale, r.cam_quat)[0].to(r.dev)
    out = {k: {"phi": at[k][0], "count": at[k][1], "directions": {}} for k in terms}
    names = ("position_x", "position_y", "position_z", "rotation_x", "rotation_y", "rotation_z", "log_scale")
    for i, name in enumerate(names):
        fd = {}
        for eps in (1e-3, 1e-4):
            fd[eps] = (phi(moved(i, eps)), phi(moved(i, -eps)))
        for k in terms:
            G = at[k][2]
            g = (M.T @ G[:8, 8]) / G[9, 9]
            rec = {"model_slope_2g": float(2 * g[i])}
            for eps, (plus, minus) in fd.items():
                rec[f"finite_difference_eps_{eps:g}"] = (plus[k][0] - minus[k][0]) / (2 * eps)
                rec[f"counts_eps_{eps:g}"] = [plus[k][1], minus[k][1]]
            rec["fd_over_model"] = rec["finite_difference_eps_0.0001"] / rec["model_slope_2g"]
            out[k]["directions"][name] = rec
            print(k, name, json.dumps(rec), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20, help="calls per sample")
    ap.add_argument("--repeats", type=int, default=9, help="interleaved rounds")
    ap.add_argument("--parts", default="kernel,iteration,convergence,gradient")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_pc_information.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pc_information.py measures on the GPU; none found")
    parts = {"kernel": kernel_part, "iteration": iteration_part, "convergence": convergence_part, "gradient": gradient_part}
    results = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            results = json.load(fh).get("results", {})
    with torch.no_grad():
        for name in a.parts.split(","):
            results[name] = parts[name](a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "image": [640, 480], "calls_per_sample": a.calls,
                   "repeats": a.repeats, "interleaved": True,
                   "what": "kernel: us per call over all views, device events; iteration: host clock around calls that end "
                           "in a device synchronise, us per iteration; convergence: Phi = mean squared depth residual + "
                           "pc_weight x mean squared point-cloud residual (m^2), its two parts measured at pc_weight = 1's "
                           "matrices whatever the run's weight, pose errors against the scene's truth; gradient: central "
                           "finite differences per unit tangent step beside 2 g of the Gram matrices; the first two samples "
                           "of every timed case are not timed",
                   "results": results}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
