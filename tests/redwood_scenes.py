"""A small annotated Redwood-style data set for the tests (test side only): the reference's directory layout and
``annotations.json`` (redwood_dataset.py:146-184) with two sequences in two categories -- a mug from the mug decoder's
marching cubes and a box of three unequal sides, both written as OBJ -- and three frames each at 160 x 120, f = 150.

``write_annotations`` needs no GPU (poses and file names only: what ``annotation(idx)`` reads); ``write_scene`` also
writes the frames.  A frame's depth is a 16-bit millimetre PNG of the rasterised mesh over a background plane at 1.5 m,
with three patches (vertical strips of the object's bounding box, over the covered pixels): one 5 cm in front of the
object (an occluder), one 5 mm in front (within the margin: not an occluder) and one of zeros (no reading).
"""
import json
import os

import numpy as np

CAMERA = dict(width=160, height=120, fx=150.0, fy=150.0, cx=80.0, cy=60.0, pixel_center=0.5)
BACKGROUND = 1.5
BOX_HALF = (0.05, 0.035, 0.08)
MUG_SCALE = 0.055
MIN_PATCH = 20


def _unit(q):
    q = np.asarray(q, dtype=np.float64)
    return (q / np.linalg.norm(q)).tolist()


# OpenCV poses (x right, y down, z forward): three per sequence
POSES = {
    "seq_mug": [([0.02, -0.01, 0.50], _unit([0.2, 0.6, -0.15, 0.75])),
                ([-0.05, 0.02, 0.55], _unit([0.7, 0.1, 0.3, 0.5])),
                ([0.06, 0.03, 0.60], _unit([-0.3, 0.5, 0.6, 0.4]))],
    "seq_box": [([0.0, 0.0, 0.60], _unit([0.3, -0.2, 0.1, 0.9])),
                ([0.08, -0.03, 0.70], _unit([0.1, 0.8, -0.2, 0.5])),
                ([-0.07, 0.02, 0.65], _unit([-0.5, 0.2, 0.4, 0.7]))],
}
CATEGORIES = {"seq_mug": "mug", "seq_box": "bottle"}


def box_obj(path, half=BOX_HALF):
    """a closed box, outward faces, as a Wavefront OBJ"""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * np.asarray(half)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    with open(path, "w") as fh:
        np.savetxt(fh, v, fmt="v %.9g %.9g %.9g")
        np.savetxt(fh, f + 1, fmt="f %d %d %d")


def write_annotations(folder, half_extents=None, poses=POSES):
    """{folder}/ann/annotations.json (and nothing else): (root_dir, ann_dir).  half_extents: {sequence: (3,)}, the
    "scale" entries (default: the box's, and a made-up one for the mug)"""
    half_extents = half_extents or {"seq_mug": [0.05, 0.04, 0.03], "seq_box": list(BOX_HALF)}
    root_dir, ann_dir = os.path.join(str(folder), "root"), os.path.join(str(folder), "ann")
    os.makedirs(ann_dir, exist_ok=True)
    anns = {}
    for seq, seq_poses in poses.items():
        anns[seq] = {"mesh": f"{seq}.obj", "category": CATEGORIES[seq], "scale": [float(x) for x in half_extents[seq]],
                     "pose_anns": [{"position": p, "orientation": q, "rgb_file": f"{n:07d}.jpg.png",
                                    "depth_file": f"{n:07d}.png"} for n, (p, q) in enumerate(seq_poses)]}
    with open(os.path.join(ann_dir, "annotations.json"), "w") as fh:
        json.dump(anns, fh)
    return root_dir, ann_dir


def write_scene(folder, camera_config=None, poses=POSES):
    """The whole set below `folder` (needs the GPU: the frames are rasterised).  Returns dict(root_dir, ann_dir,
    camera, patches): patches[i] = {"occluded", "near", "zero"} boolean (H,W) numpy arrays of sample i, in the
    dataset's sample order, each the covered pixels of its strip.  camera_config / poses: another camera, other
    frames of the two sequences (tools/bench_redwood.py: 640 x 480)."""
    import torch
    from PIL import Image
    import _loop_scenes as S
    from sdfest_amd import Camera, Mesh, extract_mesh, render_mesh_depth
    folder = str(folder)
    ann_dir = os.path.join(folder, "ann")
    os.makedirs(ann_dir, exist_ok=True)
    dec, d = S.mug_decoder()
    with torch.no_grad():
        z = torch.tensor(d["z"][9:10] * 0.5, dtype=torch.float32, device="cuda")
        mug = extract_mesh(dec.decode(z)[0, 0], 0.0, complete=True)
    mug.update_scale(MUG_SCALE, rel_scale=True)
    mug.write_obj(os.path.join(ann_dir, "seq_mug.obj"))
    box_obj(os.path.join(ann_dir, "seq_box.obj"))
    half = {}
    camera_config = dict(CAMERA if camera_config is None else camera_config)
    for seq in poses:
        v = Mesh.from_file(os.path.join(ann_dir, f"{seq}.obj"), 1.0, rel_scale=True, device="cpu").vertices.numpy()
        half[seq] = ((v.max(0) - v.min(0)) / 2).tolist()
    root_dir, ann_dir = write_annotations(folder, half, poses)
    camera = Camera(**camera_config)
    H, W = camera_config["height"], camera_config["width"]
    rng = np.random.default_rng(5)
    patches = []
    for seq, seq_poses in poses.items():
        mesh = Mesh.from_file(os.path.join(ann_dir, f"{seq}.obj"), 1.0, rel_scale=True)
        base = os.path.join(root_dir, CATEGORIES[seq], "rgbd", seq)
        os.makedirs(os.path.join(base, "rgb"), exist_ok=True)
        os.makedirs(os.path.join(base, "depth"), exist_ok=True)
        for n, (p, q) in enumerate(seq_poses):
            rendered = render_mesh_depth(mesh, camera, torch.tensor([p], dtype=torch.float32),
                                         torch.tensor([q], dtype=torch.float32), convention="open3d")[0].cpu().numpy()
            covered = rendered != 0
            ys, xs = np.nonzero(covered)
            x0, x1 = xs.min(), xs.max() + 1
            w = x1 - x0
            cols = np.arange(W)[None, :]
            strips = {"occluded": (x0, x0 + w // 4), "near": (x0 + (3 * w) // 8, x0 + (5 * w) // 8),
                      "zero": (x1 - w // 4, x1)}
            depth = np.where(covered, rendered, BACKGROUND).astype(np.float64)
            frame_patches = {}
            for name, (a, b) in strips.items():
                patch = covered & (cols >= a) & (cols < b)
                assert patch.sum() >= MIN_PATCH, (seq, n, name, int(patch.sum()))
                frame_patches[name] = patch
            depth[frame_patches["occluded"]] -= 0.05
            depth[frame_patches["near"]] -= 0.005
            depth[frame_patches["zero"]] = 0.0
            millimetres = np.round(depth * 1000.0).astype(np.uint16)
            Image.fromarray(millimetres).save(os.path.join(base, "depth", f"{n:07d}.png"))
            color = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            Image.fromarray(color).save(os.path.join(base, "rgb", f"{n:07d}.jpg.png"))
            patches.append(frame_patches)
    return dict(root_dir=root_dir, ann_dir=ann_dir, camera=camera_config, patches=patches)
