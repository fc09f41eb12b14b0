#!/usr/bin/env python3
"""Record tests/golden/mesh_record.npz: what ``render_mesh_depth``, ``mesh_to_sdf`` and ``sample_points`` give, bit for
bit, for one small table of meshes that exercises every rule of the ``sdfr_sample_mesh`` record's readers (the sort of a
face's indices and its parity, the OpenGL sign, the pose columns, which faces and records may be read).  Needs a GPU.

The file holds its own inputs and the outputs; tests/test_mesh_record_golden_gpu.py replays `compute` on the stored
inputs and compares the int32 views.  Only the public API is used, so the tool runs unchanged on any commit: record on
the commit whose bits are to be kept, never on the one under test.

Meshes: (1) ``raster_twin.cube``, every face rotated so that all six orders of an index triple occur (rotations keep
the orientation, and the cube has faces of both parities); (2) ``raster_twin.uv_sphere(8, 12)`` plus four vertices (one
NaN, three on a line) and five bad faces: an index equal to num_vertices, a negative index, a repeated index, the three
collinear vertices, the NaN vertex; (3) an empty mesh, in the depth calls only.  (2c) is mesh 2 with the NaN vertex
made finite: a NaN vertex makes ``normalize=True``'s frame and the sampler's total area NaN, so mesh 2's volume and
samples there are NaN by contract (recorded, and asserted to be NaN); the calls are repeated with 2c in its place so
that the normalised frame and the sampler also meet a mesh that is not the cube.

Usage:  python tools/make_mesh_record_goldens.py [--out tests/golden/mesh_record.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "mesh_record.npz")
W, H, F_PIX, R, N_POINTS, SEED = 48, 32, 40.0, 16, 256, 3
ORDERS = {(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)}


def unit(q):
    q = np.asarray(q, dtype=np.float64)
    return (q / np.linalg.norm(q)).astype(np.float32)


def table_inputs():
    """the meshes, poses and sizes of the table, as numpy"""
    import raster_twin as rt
    cv, cf = rt.cube(1.0)
    cf = np.stack([np.roll(f, (i // 2) % 3) for i, f in enumerate(cf)]).astype(np.int32)
    assert {tuple(np.argsort(f).tolist()) for f in cf} == ORDERS
    sv, sf = rt.uv_sphere(8, 12, 1.0)
    nv = len(sv) + 4
    extra = np.array([[np.nan, 0.1, 0.2], [0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.4, 0.4, 0.4]], np.float32)
    bad = np.array([[0, 1, nv], [-1, 2, 3], [5, 6, 5], [nv - 3, nv - 2, nv - 1], [nv - 4, 10, 11]], np.int32)
    v2 = np.concatenate([sv, extra])
    v2c = v2.copy()
    v2c[nv - 4] = (0.05, -0.1, 0.15)
    inp = {"v1": cv, "f1": cf, "v2": v2, "v2c": v2c, "f2": np.concatenate([sf, bad]),
           "scales": np.array([0.3, 0.45, 1.0], np.float32),
           # the cube's own turn is close to the third of a turn about (1, 1, 1) that maps it onto itself: at scale
           # 0.3 only a nearly grid-aligned cube centred on a grid point holds 100 of the 16^3 grid points (125 here,
           # the closest of them 4e-3 from a face); its second pose, and both of the sphere's, are general
           "quats": np.stack([unit([0.5, 0.53, 0.48, 0.51]), unit([-0.4, 0.1, 0.25, 0.85]),
                              unit([0.1, 0.2, 0.3, 0.9])]),
           # in front of the OpenGL camera (looking along -z); the Open3D calls use them with y and z negated
           "positions": np.array([[-0.25, 0.1, -1.1], [0.3, -0.15, -1.4], [0.0, 0.0, -1.0]], np.float32),
           # the second set of poses, given as tensors
           "quats_b": np.stack([unit([-0.2, 0.6, 0.1, 0.7]), unit([0.5, 0.3, -0.3, 0.75]), unit([0.0, 0.1, 0.0, 1.0])]),
           "positions_b": np.array([[0.2, -0.05, -1.2], [-0.2, 0.1, -1.3], [0.1, 0.1, -0.9]], np.float32),
           # inside the SDF volume's [-1, 1]^3
           "sdf_positions": np.array([[0.07, 0.065, -0.07], [-0.12, 0.06, -0.04]], np.float32),
           "camera": np.array([W, H, F_PIX, F_PIX, W / 2, H / 2]), "R": np.int64(R), "n_points": np.int64(N_POINTS),
           "seed": np.int64(SEED)}
    return inp


def inputs():
    """the stored inputs: the table's, and the marching-cubes mesh with vertex normals of the normals case"""
    import torch
    from sdfest_amd import extract_mesh
    from sdfest_amd.synthetic import sphere_sdf
    inp = table_inputs()
    m = extract_mesh(torch.tensor(sphere_sdf(0.5, 16), device="cuda"), 0.0, normals=True)
    inp["vn"], inp["fn"], inp["nn"] = m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.normals.cpu().numpy()
    return inp


def compute(inp):
    """every recorded output, as device tensors, from the inputs (public API only)"""
    import torch
    from sdfest_amd import Camera, Mesh, mesh_to_sdf, render_mesh_depth, sample_points
    T = lambda a, dt=torch.float32: torch.tensor(np.asarray(a), dtype=dt, device="cuda")
    w, h, fx, fy, cx, cy = (float(x) for x in inp["camera"])
    cam = Camera(int(w), int(h), fx, fy, cx, cy, pixel_center=0.5)
    scales, quats = inp["scales"], inp["quats"]

    def meshes(v2, positions, count=3):
        geo = [(inp["v1"], inp["f1"]), (v2, inp["f2"]), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))]
        return [Mesh(T(v), T(f, torch.int32), scale=float(scales[k]), rel_scale=True, position=T(positions[k]),
                     orientation=T(quats[k])) for k, (v, f) in enumerate(geo[:count])]

    out = {}
    flip = np.array([1, -1, -1], np.float32)
    for conv, sign in (("opengl", 1.0), ("open3d", flip)):
        own = meshes(inp["v2"], inp["positions"] * sign)
        out[f"depth/{conv}/own"], out[f"depth/{conv}/own_tri"] = render_mesh_depth(
            own, cam, convention=conv, return_triangles=True)
        out[f"depth/{conv}/tensors"], out[f"depth/{conv}/tensors_tri"] = render_mesh_depth(
            own, cam, T(inp["positions_b"] * sign), T(inp["quats_b"]), convention=conv, return_triangles=True)
    for tag, v2 in (("2", inp["v2"]), ("2c", inp["v2c"])):
        pair = meshes(v2, inp["sdf_positions"], 2)
        for name, kw in (("raw", dict(normalize=False)), ("norm", dict(normalize=True, padding=1))):
            if (tag, name) == ("2c", "raw"):
                continue     # no NaN there with mesh 2, and the file stays small
            key = f"sdf/{tag}/{name}"
            out[f"{key}/signed"], out[f"{key}/tri"], out[f"{key}/winding"] = mesh_to_sdf(
                pair, int(inp["R"]), signed=True, return_triangles=True, return_winding=True, **kw)
            out[f"{key}/unsigned"] = mesh_to_sdf(pair, int(inp["R"]), signed=False, **kw)
        posed = meshes(v2, inp["positions"], 2)
        for tr in (True, False):
            out[f"points/{tag}/transformed{int(tr)}"] = sample_points(posed, int(inp["n_points"]), int(inp["seed"]), tr)
    mn = Mesh(T(inp["vn"]), T(inp["fn"], torch.int32), T(inp["nn"]), scale=0.7, rel_scale=True,
              position=T(inp["positions"][0]), orientation=T(quats[0]))
    out["normals/points"], out["normals/normals"], out["normals/tri"] = mn.sample_points_uniformly(
        int(inp["n_points"]), int(inp["seed"]), normals=True, return_triangles=True)
    return out


# mesh 2's share of these is NaN (the closest face: -1) by contract: see the module docstring
NAN_BY_CONTRACT = ("sdf/2/norm/", "points/2/")


def check_not_trivial(out):
    """a golden that could not notice a change is refused: enough pixels hit, enough voxels of either sign, no output
    constant; and what is empty or NaN by contract is exactly that.  out: numpy arrays, mesh by mesh along axis 0
    (but the one mesh of the normals case)"""
    for key, a in out.items():
        group = key.split("/")[0]
        for k, part in enumerate(a[None] if group == "normals" else a):
            is_int = part.dtype.kind == "i"
            if (group == "depth" and k == 2) or (key.startswith(NAN_BY_CONTRACT) and k == 1):
                blank = -1 if is_int else (0.0 if group == "depth" else np.nan)
                assert np.array_equal(part, np.full_like(part, blank), equal_nan=True), (key, k)
                continue
            assert np.isfinite(part).all() and part.min() != part.max(), (key, k)
            if group == "depth" and not is_int:
                assert (part > 0).mean() >= 0.2, (key, k, float((part > 0).mean()))
                assert np.array_equal(part > 0, out[key + "_tri"][k] >= 0), (key, k)
            if key.endswith("/signed"):
                assert min((part < 0).sum(), (part > 0).sum()) >= 100, (key, k, int((part < 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    inp = inputs()
    out = {k: v.cpu().numpy() for k, v in compute(inp).items()}
    check_not_trivial(out)
    for k, v in compute(inp).items():
        assert np.array_equal(out[k].view(np.int32), v.cpu().numpy().view(np.int32)), f"{k}: two runs differ"
    np.savez_compressed(a.out, **{f"in/{k}": v for k, v in inp.items()}, **{f"out/{k}": v for k, v in out.items()})
    size = os.path.getsize(a.out)
    print(f"wrote {a.out}: {size} bytes, {len(inp)} inputs, {len(out)} outputs")
    assert size < 200_000, size


if __name__ == "__main__":
    main()
