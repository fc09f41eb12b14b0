#!/usr/bin/env python3
"""Objects per second of the K-object loop (``MultiObjectRenderAndCompare``) with V views per object and the inlier
bookkeeping on or off, beside the only way to do the same without it: K sequential runs of the single-estimate loop
(``FusedRenderAndCompare`` with its defaults -- what ``SDFPipeline.__call__`` runs behind the initialisation network) on
the same V views.

640x480, ``max_iterations`` 50, K in {8, 32} x V in {1, 2, 4} x tracking {off, on}.  One sample = one frame: ``rebind``
of the observation, the 50 iterations, a device synchronisation, on the host's clock.  The cases are INTERLEAVED (one
sample of every case per round, `--repeats` rounds) so that a drift of the machine meets all of them; medians and
ranges go to profiles/bench_multi_object_views.json.

The V = 1, tracking-off case uses nothing this tool's commit added: on a tree whose loop has no ``views`` argument only
that case runs (the number to compare with), and ``--today`` runs only that case on any tree, so that both numbers
come from the same interleaving.  ``--only K,V,T`` runs one side-by-side case alone, `--repeats` frames of it (the
program to put behind a kernel trace).

Memory: the side-by-side loop keeps K V volumes of SDF and 2 K V of d/dSDF (4 R^3 bytes each: 1 MiB at 64^3) and the
point clouds of K V views at capacity (12 W H bytes each): K = 32, V = 4 is 384 MiB of volumes and 450 MiB of points.
"""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def q_rot(q, v):
    return q_mul(q_mul(q, np.append(v, 0.0)), q * np.array([-1, -1, -1, 1.0]))[:3]


def scene(views, iterations, tracking):
    """the C5 object (tools/_loop_scene.py) seen from `views` cameras on an arc, 5 degrees apart, turned towards it"""
    from _loop_scene import c5_scene
    from sdfest_amd import render_depth_gpu
    s = c5_scene(views=1, max_iterations=iterations)
    dec, cam = s["decoder"], s["camera"]
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device="cuda")
    d = np.load(os.path.join(ROOT, "tests", "golden", "decoder_mug.npz"))
    p_true = np.array([0.02, -0.01, -0.5])
    q_true = np.array([0.2, 0.6, -0.15, 0.75]); q_true /= np.linalg.norm(q_true)
    cam_pos, cam_quat, depth = [], [], []
    with torch.no_grad():
        sdf = dec.decode(t(d["z"][9:10] * 0.5))[0, 0]
        for v in range(views):
            a = np.deg2rad(5.0) * v
            cam_pos.append([0.5 * np.sin(a), 0.0, -0.5 + 0.5 * np.cos(a)])
            cam_quat.append([0.0, np.sin(a / 2), 0.0, np.cos(a / 2)])
            qc = np.array(cam_quat[-1]) * np.array([-1, -1, -1, 1.0])
            depth.append(render_depth_gpu(sdf, t(q_rot(qc, p_true - np.array(cam_pos[-1]))), t(q_mul(qc, q_true)),
                                          t(1.0 / 0.055), None, None, None, 0.005, cam))
    cfg = dict(s["config"])
    if tracking:
        cfg["result_selection_strategy"] = "best_inlier_ratio"
    return dict(decoder=dec, camera=cam, config=cfg, depth=torch.stack(depth).contiguous(), cam_pos=t(cam_pos),
                cam_quat=t(cam_quat), init=s["init"])


def side_by_side(K, V, tracking, iterations, new_api):
    from sdfest_amd.pipeline import MultiObjectRenderAndCompare
    s = scene(V, iterations, tracking)
    p0, q0, s0, z0 = s["init"]
    args = (p0.expand(K, 3).contiguous(), q0.expand(K, 4).contiguous(), s0.expand(K).contiguous(),
            z0.expand(K, z0.shape[1]).contiguous())
    if V == 1 and not tracking:      # nothing but the constructor and the calls the loop has always had
        multi = MultiObjectRenderAndCompare(s["decoder"], s["camera"], s["config"], K)
        frames = s["depth"].expand(K, -1, -1).contiguous()
        bind = lambda: multi.rebind(frames)
    else:
        if not new_api:
            return None
        multi = MultiObjectRenderAndCompare(s["decoder"], s["camera"], s["config"], K, views=V)
        assert multi.track_inliers == tracking
        frames = s["depth"][None].expand(K, -1, -1, -1).contiguous()      # (K,V,H,W): every object its own images
        bind = lambda: multi.rebind(frames, s["cam_pos"], s["cam_quat"])

    def frame():
        bind()
        multi(*args)
    return frame


def sequential(K, V, tracking, iterations):
    from sdfest_amd.pipeline import FusedRenderAndCompare
    s = scene(V, iterations, tracking)
    single = FusedRenderAndCompare(s["decoder"], s["camera"], s["config"], s["depth"], s["cam_pos"], s["cam_quat"])
    assert single.track_inliers == tracking

    def frame():
        for _ in range(K):
            single.rebind(s["depth"], s["cam_pos"], s["cam_quat"])
            single(*s["init"])
    return frame


def sample(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--objects", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--views", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--today", action="store_true",
                    help="only the cases a tree without the views argument runs: the same interleaving on both trees")
    ap.add_argument("--only", help="K,V,T: that side-by-side case alone (T = 0 | 1), nothing written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_multi_object_views.json"))
    a = ap.parse_args()
    from sdfest_amd.pipeline import MultiObjectRenderAndCompare
    new_api = "views" in inspect.signature(MultiObjectRenderAndCompare.__init__).parameters and not a.today
    if a.only:
        K, V, T = (int(x) for x in a.only.split(","))
        fn = side_by_side(K, V, bool(T), a.iterations, new_api)
        ts = [sample(fn) for _ in range(a.repeats + 2)][2:]
        print(f"K={K} V={V} tracking={T}: {np.median(ts) * 1e3:.3f} ms per frame", flush=True)
        return
    cases = {}
    for K in a.objects:
        for V in a.views:
            for tracking in (False, True):
                fn = side_by_side(K, V, tracking, a.iterations, new_api)
                if fn is None:
                    continue
                cases[K, V, tracking, "side_by_side"] = fn
                cases[K, V, tracking, "sequential"] = sequential(K, V, tracking, a.iterations)
    for fn in cases.values():      # build, capture, settle
        sample(fn)
        sample(fn)
    times = {k: [] for k in cases}
    for _ in range(a.repeats):
        for k, fn in cases.items():
            times[k].append(sample(fn))
    results = []
    for (K, V, tracking, how), ts in times.items():
        if how != "side_by_side":
            continue
        seq = times[K, V, tracking, "sequential"]
        row = {"objects": K, "views": V, "tracking": tracking}
        for name, t in (("side_by_side", ts), ("sequential", seq)):
            row[name] = {"objects_per_s": K / float(np.median(t)), "median_ms": float(np.median(t)) * 1e3,
                         "min_ms": float(min(t)) * 1e3, "max_ms": float(max(t)) * 1e3}
        row["ratio"] = row["side_by_side"]["objects_per_s"] / row["sequential"]["objects_per_s"]
        results.append(row)
        print(f"K={K:2d} V={V} tracking={'on ' if tracking else 'off'}: side by side "
              f"{row['side_by_side']['objects_per_s']:8.1f} objects/s ({row['side_by_side']['median_ms']:8.3f} ms "
              f"[{row['side_by_side']['min_ms']:.3f}, {row['side_by_side']['max_ms']:.3f}]), one at a time "
              f"{row['sequential']['objects_per_s']:7.1f} objects/s: {row['ratio']:.2f}x", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "image": [640, 480], "iterations": a.iterations,
                   "repeats": a.repeats, "interleaved": True, "loop_has_views_argument": new_api, "results": results},
                  fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
