#!/usr/bin/env python3
"""What looking at a run costs: ``sdfr_render_normals`` and ``sdfr_shade_frames`` (csrc/shade.hip) on the device.

Part 1: 256 frames of 640x480 on the benchmark views (bench.py's scene: blobs(0), random_poses(256, seed 1)) --
``render_normals`` and ``shade_frames`` with all three outputs (and with the two colour-mapped ones alone, and the
shaded one alone), beside the forward render of the same frames (``sdfr_render_forward``, which this feature does not
touch: the number is this commit's parent's) and beside device-to-device copies of the bytes each pass must move
(``Tensor.copy_``: that many bytes read and as many written; a pass that reads r and writes w bytes is set beside a
copy of (r + w) / 2).  Bytes are counted from shapes: normals read 4 and write 12 per pixel; shading reads 4 (depth) + 4
(target) and writes 3 per output; the grid gathers of hit pixels are served by the L2 and are not counted.
Part 2: the front door -- a 50-iteration ``SDFPipeline`` call on one 640x480 view of the mug decoder (``step_log``
on), ``render_trajectory()`` of its 51 states, the copy of the three frame streams to the host, and the host's PNG
encoding of them (``write_frames``) and GIF encoding (``write_animation``), host clock around a synchronise.
A device sample is `--calls` consecutive calls between two device events; everything is warmed up and the samples are
INTERLEAVED (`--repeats` rounds).  Medians and ranges go to profiles/bench_shading.json."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_boxes import event_sample, host_sample, interleaved, stat   # noqa: E402


def kernel_part(a):
    from sdfest_amd import Camera, depth_range, render_normals, shade_frames
    from sdfest_amd.differentiable_renderer import forward_raw
    from sdfest_amd.synthetic import blobs_sdf, random_poses
    dev = torch.device("cuda:0")
    B, W, H, thr = a.frames, 640, 480, 0.005
    cam = Camera(W, H, W / 2.0, W / 2.0, W / 2.0, H / 2.0, pixel_center=0.5)
    sdf = torch.tensor(blobs_sdf(0), device=dev)
    pos, quat, isc = (torch.tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)
                      for x in random_poses(B, seed=1, width=W, height=H, f=W / 2.0))
    fx, fy, cx, cy, _ = cam.get_pinhole_camera_parameters(0.5)
    forward = lambda: forward_raw(sdf, pos, quat, isc, W, H, cx, cy, fx, fy, thr)
    depth = forward()
    target = (depth[:1] * 1.01).contiguous()
    rng = depth_range(depth, shared=True)
    px = B * W * H
    traffic = {"normals": (4 * px, 12 * px), "shade_all": (8 * px, 9 * px), "shade_maps": (8 * px, 6 * px),
               "shade_shaded": (4 * px, 3 * px)}
    buffers = {k: (torch.empty((r + w) // 2, dtype=torch.uint8, device=dev),
                   torch.empty((r + w) // 2, dtype=torch.uint8, device=dev)) for k, (r, w) in traffic.items()}
    shade = lambda names: shade_frames(depth, sdf, pos, quat, isc, cam, target=target, value_range=rng, outputs=names)
    passes = {"forward": forward,
              "normals": lambda: render_normals(sdf, pos, quat, isc, thr, cam, depth=depth),
              "shade_all": lambda: shade(("depth", "depth_error", "shaded")),
              "shade_maps": lambda: shade(("depth", "depth_error")),
              "shade_shaded": lambda: shade(("shaded",)),
              "depth_range_per_frame": lambda: depth_range(depth),
              "depth_range_shared": lambda: depth_range(depth, shared=True)}
    for k, (src, dst) in buffers.items():
        passes["copy_" + k] = (lambda s=src, d=dst: d.copy_(s))
    samplers = {k: (lambda f=f: event_sample(f, a.calls)) for k, f in passes.items()}
    ts = interleaved(samplers, a.repeats)
    out = {"frames": B, "width": W, "height": H, "hit_share": float((depth != 0).float().mean())}
    for k in passes:
        out[k] = stat(ts[k])
    for k, (r, w) in traffic.items():
        t, c = float(np.median(ts[k])), float(np.median(ts["copy_" + k]))
        out[k].update({"bytes_read": r, "bytes_written": w, "GBps": (r + w) / t * 1e-9,
                       "copy_GBps": (r + w) / c * 1e-9, "share_of_copy_rate": c / t})
    out["shade_all"]["of_forward"] = float(np.median(ts["shade_all"]) / np.median(ts["forward"]))
    out["normals"]["of_forward"] = float(np.median(ts["normals"]) / np.median(ts["forward"]))
    print(json.dumps(out, indent=1))
    return out


def front_door_part(a):
    from test_sdfpipeline_gpu import T, make_config, mug_weights, plausible_init_state
    from sdfest_amd import SDFPipeline, write_animation, write_frames
    W, H, n_iter = 640, 480, 50
    cfg = make_config(W, H, 600.0, 600.0, 320.0, 240.0, 0.005, n_iter, far_field=2.0, step_log=True)
    pipe = SDFPipeline(cfg, vae_state_dict=mug_weights(), init_state_dict=plausible_init_state())
    d = np.load(os.path.join(ROOT, "tests", "golden", "decoder_mug.npz"))
    q = T([0.2, 0.6, -0.15, 0.75])
    with torch.no_grad():
        scene = pipe.generate_depth(T([0.02, -0.01, -0.5]), q / q.norm(), T(0.055), T(d["z"][9:10]) * 0.5)
    mask = scene > 0
    color = torch.zeros((H, W, 3), device="cuda")
    call = lambda: pipe(scene.clone(), mask, color)
    call()
    frames = pipe.render_trajectory()
    host = {k: v.cpu() for k, v in frames.items()}
    folder = tempfile.mkdtemp(prefix="bench_shading_")

    def encode_png():
        for k, v in host.items():
            write_frames(os.path.join(folder, k), v[1:])

    def encode_gif():
        for k, v in host.items():
            write_animation(os.path.join(folder, k + ".gif"), v[1:])

    samplers = {"call_50_iterations": lambda: host_sample(call, 2),
                "render_trajectory": lambda: host_sample(pipe.render_trajectory, 4),
                "frames_to_host": lambda: host_sample(lambda: [v.cpu() for v in frames.values()], 2)}
    ts = interleaved(samplers, a.repeats)
    out = {"width": W, "height": H, "iterations": n_iter, "states": int(frames["depth"].shape[0]),
           "hit_pixels": int(mask.sum())}
    for k in samplers:
        out[k] = stat(ts[k], "ms")
    for name, fn in (("png_encoding_150_frames", encode_png), ("gif_encoding_3_streams", encode_gif)):
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        out[name] = stat(t, "ms")
    out["render_trajectory_of_call"] = float(np.median(ts["render_trajectory"]) / np.median(ts["call_50_iterations"]))
    print(json.dumps(out, indent=1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--calls", type=int, default=8, help="calls per device sample")
    ap.add_argument("--repeats", type=int, default=11, help="interleaved rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_shading.json"))
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "repeats": a.repeats,
              "kernels": kernel_part(a), "front_door": front_door_part(a)}
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("written", a.out)


if __name__ == "__main__":
    main()
