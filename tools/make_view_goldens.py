#!/usr/bin/env python3
"""Capture tests/golden/eval_views.npz by IMPORTING the reference's sdfest/initialization/quaternion_utils.py (torch
only; loaded by file path): the camera algebra of estimation/scripts/rendering_evaluation.py::_generate_views, lines
207-231, for a few seeded camera quaternions and mesh orientations -- numbers only.

For every case: the camera orientation (OpenGL camera to world, the input), the mesh's world orientation and the
camera distance (inputs); the camera position in the world (the object on the principal axis) and the mesh's
orientation in the Open3D camera frame (outputs).  The mesh's position in that frame is (0, 0, camera_distance).

Usage:  python tools/make_view_goldens.py --ref <checkout of the reference>
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "eval_views.npz")


def load_quaternion_utils(ref):
    path = os.path.join(ref, "sdfest/initialization/quaternion_utils.py")
    spec = importlib.util.spec_from_file_location("ref_quaternion_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference repository")
    args = ap.parse_args()
    qu = load_quaternion_utils(args.ref)
    rng = np.random.default_rng(2024)
    n = 12
    cam_q = rng.normal(size=(n, 4))
    cam_q /= np.linalg.norm(cam_q, axis=1, keepdims=True)
    cam_q[0] = [0, 0, 0, 1]
    cam_q[1] = [1, 0, 0, 0]
    mesh_q = rng.normal(size=(n, 4))
    mesh_q /= np.linalg.norm(mesh_q, axis=1, keepdims=True)
    mesh_q[:3] = [0, 0, 0, 1]
    dist = rng.uniform(0.3, 1.2, n)
    cam_pos, mesh_q_cam = [], []
    for i in range(n):
        camera_orientation = torch.tensor(cam_q[i], dtype=torch.float64)
        mesh_orientation = torch.tensor(mesh_q[i], dtype=torch.float64)
        mesh_position = torch.zeros(3, dtype=torch.float64)
        # the lines of _generate_views, with the reference's own functions
        camera_position = mesh_position - qu.quaternion_apply(
            camera_orientation, torch.tensor([0, 0, -dist[i]], dtype=torch.float64))
        camera_orientation_o3d = qu.quaternion_multiply(camera_orientation,
                                                        torch.tensor([1.0, 0, 0, 0], dtype=torch.float64))
        mesh_orientation_cam = qu.quaternion_multiply(qu.quaternion_invert(camera_orientation_o3d), mesh_orientation)
        cam_pos.append(camera_position.numpy())
        mesh_q_cam.append(mesh_orientation_cam.numpy())
    np.savez(OUT, camera_orientations=cam_q, mesh_orientations=mesh_q, camera_distances=dist,
             camera_positions=np.stack(cam_pos), mesh_orientations_cam=np.stack(mesh_q_cam))
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
