#!/usr/bin/env python3
"""What the Levenberg-Marquardt refinement costs and what it buys (the method of tools/bench_information.py: warmed up,
samples INTERLEAVED over `--repeats` rounds, a sample being `--calls` consecutive calls).

Part 1, kernel against the host path: ``sdfr_lm_step`` alone (the init form: accept, copy, project, solve, retract) for
K in {1, 32, 1024} objects of V = 2 views at T = 0 and T = 8, beside the float64 torch path that existed before it --
``tangent_information`` / ``joint_tangent_information``, the sum over an object's views and a batched
``torch.linalg.solve`` of the damped system on the same matrices.  Device events for the kernel, and the host clock
around calls that end in a device synchronise for both (the torch path is host-bound).
Part 2, one LM iteration end to end (``LMRefiner.iterate(1)``: decode, render, [JVP,] Gram matrices, step, poses) on
the C5 mug scene at 640x480, pose only and with shape, K = 1 and K = 32, beside one iteration of the captured Adam loop
on the same scene (a run of `--iterations` iterations over their number).
Part 3, convergence: Phi = mean r^2 and the pose error after 50 Adam iterations, after 50 Adam + 5 LM and after 10 Adam
+ 10 LM, from the perturbed start of the C5 scene and (Phi only: the golden holds no truth) from G7 run C's start, with
``pose_uncertainty().position_std`` before and after ``refine``.
Part 4, the model against the objective: central finite differences of Phi along the seven pose tangent directions at
the C5 start (each a re-render through ``LMRefiner.evaluate``) beside the model's slope 2 g from the Gram matrices at
that start.
Everything goes to profiles/bench_lm.json as found (a run of some `--parts` replaces those parts of an existing file);
none of it is a test gate."""
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

from bench_information import event_sample, host_sample, stat  # noqa: E402
from bench_shape_information import interleaved, report  # noqa: E402


def kernel_part(a):
    from sdfest_amd import joint_tangent_information, lm, tangent_information
    dev = torch.device("cuda:0")
    V, lam = 2, 1e-3
    out = {}
    for T in (0, 8):
        for K in (1, 32, 1024):
            F, n = 10 + T, 7 + T
            g = torch.Generator(device="cpu").manual_seed(K * 100 + T)
            f = torch.randn((K * V, 60, F), generator=g, dtype=torch.float64)
            f[..., 9 + T] = 1.0
            gram = (f.transpose(1, 2) @ f).to(dev).contiguous()
            rows = torch.randn((K, 8 + T), generator=g)
            rows[:, 7] = 0.1 + rows[:, 7].abs() * 0.05
            rows = rows.to(dev)
            cq = torch.randn((V, 4), generator=g)
            cq = (cq / cq.norm(dim=1, keepdim=True)).to(dev)
            pt, pc, gc = rows.clone(), torch.empty_like(rows), torch.empty_like(gram)
            state = torch.empty((K, lm.STATE_DOUBLES), dtype=torch.float64, device=dev)
            step = torch.empty((K, n), dtype=torch.float64, device=dev)

            def kernel():
                pt.copy_(rows)
                lm.lm_step(gram, pt, pc, gc, state, cq, V, True, step=step, lambda0=lam)

            def host():
                q = rows[:, 3:7] / rows[:, 3:7].norm(dim=1, keepdim=True)
                w2c = cq * cq.new_tensor([-1.0, -1.0, -1.0, 1.0])
                from sdfest_amd.pipeline import quaternion_multiply
                q_c = quaternion_multiply(w2c[None].expand(K, V, 4), q[:, None].expand(K, V, 4)).reshape(K * V, 4)
                isc = (1.0 / rows[:, 7])[:, None].expand(K, V).reshape(K * V)
                cams = cq[None].expand(K, V, 4).reshape(K * V, 4)
                if T:
                    Hv = joint_tangent_information(gram, q_c, isc, cams)
                else:
                    Hv = tangent_information(gram, q_c, isc, cams)
                cnt = gram[:, 9 + T, 9 + T].reshape(K, V).sum(1)
                H = Hv.reshape(K, V, n, n).sum(1) / cnt[:, None, None]
                # (the gradient's projection is part of neither function: its cost is left out in the host path's favour)
                gvec = gram[:, :n, 8 + T].reshape(K, V, n).sum(1) / cnt[:, None]
                d = torch.diagonal(H, dim1=-2, dim2=-1)
                A = H + lam * torch.diag_embed(torch.maximum(d, 1e-12 * d.max(dim=1, keepdim=True).values))
                return torch.linalg.solve(A, -gvec)

            kernel()
            host()
            key = f"K{K}_T{T}"
            ev = interleaved({f"{key}_kernel_events": kernel}, event_sample, a.calls, a.repeats)
            times = interleaved({f"{key}_kernel": kernel, f"{key}_host_path": host}, host_sample, a.calls, a.repeats)
            times.update(ev)
            out.update(report(times, "us"))
            out[f"{key}_host_over_kernel"] = float(np.median(times[f"{key}_host_path"]) / np.median(times[f"{key}_kernel"]))
            print(f"{key}: host path / kernel = {out[f'{key}_host_over_kernel']:.1f}", flush=True)
    return out


def iteration_part(a):
    from _loop_scene import c5_scene
    from sdfest_amd import LMRefiner
    from sdfest_amd.pipeline import FusedRenderAndCompare, MultiObjectRenderAndCompare
    sc = c5_scene(views=1, max_iterations=a.iterations)
    dec, cam, cfg, init = sc["decoder"], sc["camera"], sc["config"], sc["init"]
    row = torch.cat([init[0], init[1], init[2][:, None], init[3]], dim=1)
    out = {}
    for K in (1, 32):
        cases = {}
        target = sc["targets"][:1].repeat(K, 1, 1).contiguous()
        for shape in (False, True):
            r = LMRefiner((dec, cam, cfg["threshold"]), K, 1, shape).start(row.repeat(K, 1), target)
            r.iterate(2)
            cases[f"K{K}_lm_iteration_{'shape' if shape else 'pose'}"] = lambda r=r: r.iterate(1)
            if K == 1:
                loop = FusedRenderAndCompare(dec, cam, cfg, target, shape_optimization=shape)
                args = init
            else:
                loop = MultiObjectRenderAndCompare(dec, cam, cfg, K, shape_optimization=shape).rebind(target)
                args = tuple(t.repeat(K, *([1] * (t.dim() - 1))) for t in init)
            loop(*args)
            cases[f"K{K}_adam_run_{'shape' if shape else 'pose'}"] = lambda loop=loop, args=args: loop(*args)
        times = interleaved(cases, host_sample, max(1, a.calls // 4), a.repeats)
        for k in list(times):
            if "_adam_run_" in k:     # a run of `iterations` iterations -> one iteration
                times[k.replace("_adam_run_", "_adam_iteration_")] = [t / a.iterations for t in times.pop(k)]
        out.update(report(times, "us"))
        for s in ("pose", "shape"):
            out[f"K{K}_lm_over_adam_iteration_{s}"] = (out[f"K{K}_lm_iteration_{s}"]["median_us"]
                                                       / out[f"K{K}_adam_iteration_{s}"]["median_us"])
            print(f"K={K} {s}: LM iteration / Adam iteration = {out[f'K{K}_lm_over_adam_iteration_{s}']:.1f}", flush=True)
    return out


def pose_error(rows, truth):
    rows, truth = np.asarray(rows, np.float64), np.asarray(truth, np.float64)
    c = abs(np.dot(rows[3:7] / np.linalg.norm(rows[3:7]), truth[3:7] / np.linalg.norm(truth[3:7])))
    return {"position_mm": float(np.linalg.norm(rows[:3] - truth[:3]) * 1e3),
            "rotation_deg": float(np.degrees(2 * np.arccos(min(1.0, c)))), "scale_rel": float(abs(rows[7] / truth[7] - 1.0))}


def convergence_part(a):
    from _loop_scene import c5_scene
    from bench_hypotheses import pipeline
    out = {}

    def schedule(make, run, truth, name):
        for adam, lm_n in ((50, 0), (50, 5), (10, 10)):
            pipe = make(adam)
            run(pipe)
            before = pipe.pose_uncertainty().position_std[0].tolist()
            est, rep = pipe.refine(lm_n)
            after = pipe.pose_uncertainty().position_std[0].tolist()
            rows = torch.cat([est[0], est[1], est[2][:, None], est[3]], dim=1)[0].cpu().numpy()
            rec = {"phi_after_adam": float(rep.initial_cost[0]), "phi_final": float(rep.final_cost[0]),
                   "accepted": int(rep.accepted[0]), "rejected": int(rep.rejected[0]), "status": int(rep.status[0]),
                   "final_lambda": float(rep.final_lambda[0]), "count": float(rep.final_count[0]),
                   "position_std_before": before, "position_std_after": after,
                   "position_std_ratio": [y / x if x else None for x, y in zip(before, after)]}
            if truth is not None:
                rec["pose_error"] = pose_error(rows, truth)
            out[f"{name}_adam{adam}_lm{lm_n}"] = rec
            print(name, adam, lm_n, json.dumps(rec), flush=True)

    # the perturbed start of the C5 scene
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

    # G7 run C: two views at 160x120, shape optimisation on, from the golden's start
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
    r = LMRefiner((sc["decoder"], sc["camera"], sc["config"]["threshold"]), 1, 1, False).start(row, sc["targets"][:1])

    def phi(rows):
        r.params_trial.copy_(rows)
        r._poses(_stream(r.dev))
        r.evaluate()
        G = r.gram_trial[0]
        return float(G[8, 8] / G[9, 9]), float(G[9, 9]), G.clone()

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

    phi0, cnt0, G = phi(row)
    M = tangent_map(r.quat_c, r.inv_scale, r.cam_quat)[0].to(G.device)
    g = (M.T @ G[:8, 8]) / G[9, 9]
    out = {"phi": phi0, "count": cnt0, "directions": {}}
    names = ("position_x", "position_y", "position_z", "rotation_x", "rotation_y", "rotation_z", "log_scale")
    for i, name in enumerate(names):
        rec = {"model_slope_2g": float(2 * g[i])}
        for eps in (1e-3, 1e-4):
            (pp, cp, _), (pm, cm, _) = phi(moved(i, eps)), phi(moved(i, -eps))
            rec[f"finite_difference_eps_{eps:g}"] = (pp - pm) / (2 * eps)
            rec[f"counts_eps_{eps:g}"] = [cp, cm]
        rec["fd_over_model"] = rec["finite_difference_eps_0.0001"] / rec["model_slope_2g"]
        out["directions"][name] = rec
        print(name, json.dumps(rec), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iterations", type=int, default=50, help="iterations of the Adam run an iteration's time is taken from")
    ap.add_argument("--calls", type=int, default=20, help="calls per sample")
    ap.add_argument("--repeats", type=int, default=9, help="interleaved rounds")
    ap.add_argument("--parts", default="kernel,iteration,convergence,gradient")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_lm.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm.py measures on the GPU; none found")
    parts = {"kernel": kernel_part, "iteration": iteration_part, "convergence": convergence_part,
             "gradient": gradient_part}
    results = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            results = json.load(fh).get("results", {})
    with torch.no_grad():
        for name in a.parts.split(","):
            results[name] = parts[name](a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "image": [640, 480], "adam_iterations_per_run": a.iterations,
                   "calls_per_sample": a.calls, "repeats": a.repeats, "interleaved": True,
                   "what": "kernel: us per call, device events (_events) and the host clock around calls that end in a "
                           "device synchronise; iteration: host clock, us per iteration; convergence: Phi = mean squared "
                           "depth residual (m^2) and pose errors against the scene's truth; gradient: central finite "
                           "differences of Phi per unit tangent step beside 2 g of the Gram matrices; the first two "
                           "samples of every timed case are not timed",
                   "results": results}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
