"""GPU: marching cubes (sdfr_mesh_count / sdfr_mesh_emit, sdfest_amd.mesh) against the CPU twin tests/mesh_twin.py --
the same vertex and face lists, bit-identical runs, batches equal to single calls -- and ``SDFPipeline.generate_mesh`` /
``generate_meshes`` on the mug decoder (simple_setup.py:621-669)."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN
import mesh_twin as mt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tabs():
    return mt.tables()


def fields():
    from sdfest_amd.synthetic import sphere_sdf
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    noise = np.random.default_rng(0).uniform(-1, 1, (32, 32, 32)).astype(np.float32)
    return {"sphere": (sphere_sdf(0.5, 64), 0.0), "mug": (d["z0_full"], 0.02), "noise": (noise, 0.0)}


@pytest.mark.parametrize("complete", [False, True])
@pytest.mark.parametrize("name", ["sphere", "mug", "noise"])
def test_kernel_equals_twin(tabs, name, complete):
    from sdfest_amd import extract_mesh
    sdf, level = fields()[name]
    m = extract_mesh(torch.tensor(sdf, device="cuda"), level, complete=complete, normals=True)
    v, f, n = mt.marching_cubes(sdf, level, complete=complete, normals=True, tabs=tabs)
    gv, gf, gn = m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.normals.cpu().numpy()
    assert gv.shape == v.shape and gf.shape == f.shape
    assert m.faces.dtype == torch.int32 and m.vertices.dtype == torch.float32
    assert np.array_equal(gf, f)
    assert np.abs(gv - v).max() <= 1e-6
    # normals: 1e-5, and where the lerped gradient nearly vanishes the float32 rounding of its components is amplified
    # by 1 / |gradient| (white noise has such vertices); the twin's unnormalised length bounds it
    err = np.abs(gn - n).max(1)
    assert np.all(err <= 1e-5 + 1e-6 / np.maximum(_twin_gradient_norm(sdf, level, complete), 1e-30)), err.max()
    if name == "sphere":
        assert len(np.unique(gf)) == len(gv)


def _twin_gradient_norm(sdf, level, complete):
    """|lerped gradient| at every twin vertex (the length the normal is divided by)"""
    v = mt.padded(sdf, complete)
    lvl = np.float32(level)
    inside = v < lvl
    M = v.shape[0]
    crossed = np.zeros((M, M, M, 3), dtype=bool)
    crossed[:-1, :, :, 0] = inside[:-1] != inside[1:]
    crossed[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    crossed[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    g, a = np.nonzero(crossed.reshape(-1, 3))
    idx = np.stack(np.unravel_index(g, (M, M, M)), 1)
    other = idx.copy()
    other[np.arange(len(a)), a] += 1
    va, vb = v[tuple(idx.T)].astype(np.float64), v[tuple(other.T)].astype(np.float64)
    t = (np.float64(lvl) - va) / (vb - va)
    grads = np.stack(np.gradient(v.astype(np.float64)), -1)
    gn = grads[tuple(idx.T)] + t[:, None] * (grads[tuple(other.T)] - grads[tuple(idx.T)])
    return np.linalg.norm(gn, axis=1)


def test_two_calls_are_bitwise_identical():
    from sdfest_amd import extract_mesh
    sdf, level = fields()["noise"]
    x = torch.tensor(sdf, device="cuda")
    a = extract_mesh(x, level, complete=True, normals=True)
    b = extract_mesh(x, level, complete=True, normals=True)
    assert torch.equal(a.faces, b.faces)
    assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))
    assert torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32))


@pytest.mark.parametrize("complete", [False, True])
def test_batch_equals_single_calls(complete):
    from sdfest_amd import extract_mesh
    from sdfest_amd.synthetic import blobs_sdf, sphere_sdf
    grids = [blobs_sdf(s, R=40) for s in range(3)] + [sphere_sdf(0.3, 40), sphere_sdf(0.7, 40)]
    x = torch.tensor(np.stack(grids), device="cuda")
    batch = extract_mesh(x, 0.01, complete=complete, normals=True)
    batch5 = extract_mesh(x[:, None], 0.01, complete=complete, normals=True)      # (N,1,R,R,R) as decode returns
    assert len(batch) == 5
    for n in range(5):
        one = extract_mesh(x[n], 0.01, complete=complete, normals=True)
        for m in (batch[n], batch5[n]):
            assert torch.equal(m.faces, one.faces)
            assert torch.equal(m.vertices.view(torch.int32), one.vertices.view(torch.int32))
            assert torch.equal(m.normals.view(torch.int32), one.normals.view(torch.int32))
    assert len({int(m.vertices.shape[0]) for m in batch}) == 5


def test_sphere_normals_match_the_analytic_normal():
    from sdfest_amd import extract_mesh
    from sdfest_amd.synthetic import sphere_sdf
    for complete in (False, True):
        m = extract_mesh(torch.tensor(sphere_sdf(0.5, 64), device="cuda"), 0.0, complete=complete, normals=True)
        v, n = m.vertices.double(), m.normals.double()
        radial = v / v.norm(dim=1, keepdim=True)
        assert float((radial * n).sum(1).min()) >= 0.999      # twin: 0.9999996
        assert float((n.norm(dim=1) - 1).abs().max()) < 1e-5


def test_level_outside_the_data_range_raises():
    from sdfest_amd import extract_mesh
    from sdfest_amd.synthetic import sphere_sdf
    x = torch.tensor(sphere_sdf(0.5, 32), device="cuda")
    lo, hi = float(x.min()), float(x.max())
    with pytest.raises(ValueError):
        extract_mesh(x, hi + 0.1)
    with pytest.raises(ValueError):
        extract_mesh(x, lo - 0.1)
    with pytest.raises(ValueError):      # a batch raises for any grid out of range
        extract_mesh(torch.stack([x, x + 10.0]), 0.0)
    # the padding's 1.0 counts towards the range, as for the reference's padded volume
    m = extract_mesh(x - 5.0, 0.5, complete=True)
    assert m.faces.shape[0] > 0


def test_empty_mesh_when_no_edge_crosses():
    from sdfest_amd import extract_mesh
    x = torch.full((16, 16, 16), 0.5, device="cuda")
    m = extract_mesh(x, 0.5)
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3)


def make_pipeline(**extra):
    from sdfest_amd import SDFPipeline
    from test_sdfpipeline_gpu import make_config, mug_weights

    def no_init(*args):
        raise AssertionError("not used")

    cfg = make_config(160, 120, 100.0, 100.0, 80.0, 60.0, 0.005, 2, **extra)
    return SDFPipeline(cfg, vae_state_dict=mug_weights(), init_network=no_init), cfg


@pytest.fixture(scope="module")
def mug_z():
    return np.load(os.path.join(GOLDEN, "decoder_mug.npz"))["z"]


def test_generate_mesh_on_the_mug(mug_z):
    from sdfest_amd import Mesh, extract_mesh
    pipe, cfg = make_pipeline()
    z = torch.tensor(mug_z[:1], device="cuda")
    scale = torch.tensor([0.07], device="cuda")
    for complete in (False, True):
        mesh = pipe.generate_mesh(z, scale, complete_mesh=complete)
        assert isinstance(mesh, Mesh) and mesh.rel_scale and mesh.scale == pytest.approx(0.07)
        ref = extract_mesh(pipe.vae.decode(z)[0, 0], cfg["iso_threshold"], complete=complete)
        assert torch.equal(mesh.faces, ref.faces)
        assert torch.equal(mesh.vertices, ref.vertices)
        assert torch.equal(mesh.scaled_vertices(), ref.vertices * np.float32(0.07).item())
        assert mesh.faces.shape[0] > 1000
    # pose: R(q) (s v) + p
    mesh.position = torch.tensor([0.1, -0.2, 0.3], device="cuda")
    mesh.orientation = torch.tensor([0.0, 0.0, np.sin(np.pi / 4), np.cos(np.pi / 4)], device="cuda")   # 90 deg about z
    sv, tv = mesh.scaled_vertices(), mesh.transformed_vertices()
    expect = torch.stack([-sv[:, 1], sv[:, 0], sv[:, 2]], 1) + mesh.position
    assert float((tv - expect).abs().max()) < 1e-6


def test_generate_mesh_without_iso_threshold_returns_none(mug_z):
    pipe, cfg = make_pipeline()
    del pipe.config["iso_threshold"]
    z = torch.tensor(mug_z[:1], device="cuda")
    assert pipe.generate_mesh(z, torch.tensor([0.1], device="cuda")) is None
    assert pipe.generate_meshes(torch.tensor(mug_z[:2], device="cuda"), torch.tensor([0.1, 0.2], device="cuda")) is None


def test_generate_meshes_equals_generate_mesh(mug_z):
    from sdfest_amd import extract_mesh
    pipe, _ = make_pipeline()
    z = torch.tensor(mug_z[:3], device="cuda")
    scales = torch.tensor([0.05, 0.08, 0.11], device="cuda")
    for complete in (False, True):
        meshes = pipe.generate_meshes(z, scales, complete_mesh=complete)
        assert len(meshes) == 3
        same = extract_mesh(pipe.vae.decode(z), pipe.config["iso_threshold"], complete=complete)
        for k in range(3):
            assert torch.equal(meshes[k].faces, same[k].faces) and torch.equal(meshes[k].vertices, same[k].vertices)
            one = pipe.generate_mesh(z[k:k + 1], scales[k:k + 1], complete_mesh=complete)
            # the batched decode may take other, equivalent decoder kernels than a single latent (equal to rounding):
            # the same triangles, the positions to rounding
            assert torch.equal(meshes[k].faces, one.faces)
            assert meshes[k].scale == one.scale
            assert float((meshes[k].vertices - one.vertices).abs().max()) < 1e-5


def test_write_obj_and_ply_round_trip(tmp_path):
    from sdfest_amd import extract_mesh
    from sdfest_amd.synthetic import sphere_sdf
    m = extract_mesh(torch.tensor(sphere_sdf(0.5, 24), device="cuda"), 0.0, complete=True, normals=True)
    m.update_scale(0.5, rel_scale=True)
    path = tmp_path / "m.obj"
    m.write_obj(str(path))
    vs, vns, fs = [], [], []
    for line in open(path):
        tok = line.split()
        if not tok or tok[0] == "#":
            continue
        if tok[0] == "v":
            vs.append([float(x) for x in tok[1:4]])
        elif tok[0] == "vn":
            vns.append([float(x) for x in tok[1:4]])
        elif tok[0] == "f":
            fs.append([int(x.split("/")[0]) - 1 for x in tok[1:4]])
    v, f, n = m.numpy()
    assert np.array_equal(np.array(fs), f)
    assert np.abs(np.array(vs) - v).max() <= 1e-7 and np.abs(np.array(vns) - n).max() <= 1e-7
    ply = tmp_path / "m.ply"
    m.write_ply(str(ply))
    raw = open(ply, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert f"element vertex {len(v)}".encode() in head and f"element face {len(f)}".encode() in head
    vert = np.frombuffer(body[:len(v) * 24], dtype="<f4").reshape(-1, 6)
    face = np.frombuffer(body[len(v) * 24:], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    assert np.array_equal(vert[:, :3], v) and np.array_equal(vert[:, 3:], n)
    assert (face["n"] == 3).all() and np.array_equal(face["i"], f)
