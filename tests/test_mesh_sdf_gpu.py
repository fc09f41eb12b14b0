"""GPU: mesh -> SDF volume (``sdfr_mesh_sdf``, csrc/mesh_sdf.hip, ``sdfest_amd.mesh_to_sdf``) against its float64 CPU
twin tests/mesh_sdf_twin.py, against marching cubes (separation, round trip), its bitwise promises, the normalised
framing, ``evaluation.vae_reconstruction`` and ``tools/process_meshes.py``.

There is no golden from the reference: its mesh_to_sdf package (and trimesh, pyrender) cannot run here, and its
scan-based values approximate what this computes exactly.  The distance tolerance of a scene is 4 x the largest error
the float32 twin makes against the float64 twin on that scene's sample (the margin of DESIGN.md section 3.12), with a
floor of 2 ulp of the grid's extent (2.0)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import mesh_sdf_twin as mst
import raster_twin as rt
from helpers import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

T = lambda a, dt=torch.float32: torch.tensor(np.asarray(a), dtype=dt, device="cuda")
FLOOR = 2 * float(np.spacing(np.float32(2.0)))
IDENTITY = (1.0, (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))


def gpu_mesh(mesh, pose=IDENTITY):
    from sdfest_amd import Mesh
    v, f = mesh
    factor, quat, position = pose
    return Mesh(T(v), T(f, torch.int32), scale=factor, rel_scale=True, position=T(position), orientation=T(quat))


def unit(q):
    q = np.asarray(q, dtype=np.float64)
    return tuple(float(c) for c in (q / np.linalg.norm(q)).astype(np.float32))


def offcentre_sphere(R=64, centre=(0.1, -0.05, 0.08), radius=0.55):
    ax = np.linspace(-1.0, 1.0, R)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - radius).astype(np.float32)


def mc_mesh(grid, level, complete):
    from sdfest_amd import extract_mesh
    return extract_mesh(T(grid), level, complete=complete)


def blobs():
    from sdfest_amd.synthetic import blobs_sdf
    return blobs_sdf(0)


def parity_scene(name):
    """(vertices, faces) as numpy, pose, closed"""
    if name == "sphere":
        return rt.uv_sphere(24, 32, 0.7), IDENTITY, True
    if name == "torus":
        return mst.torus(40, 20, 0.6, 0.25), IDENTITY, True
    if name == "posed_box":
        pose = (float(np.float32(0.45)), unit([0.31, -0.52, 0.2, 0.77]), (0.1, -0.05, 0.08))
        return rt.cube(1.0), tuple(pose), True
    if name == "open_bowl":
        return mst.bowl(), IDENTITY, False
    if name == "blobs_mc":
        m = mc_mesh(blobs(), 0.0, False)
        return (m.vertices.cpu().numpy(), m.faces.cpu().numpy()), IDENTITY, True
    raise KeyError(name)


def distance_tolerance(pts, mesh, pose):
    d64 = mst.evaluate(pts, *mesh, pose=pose, signed=False)[0]
    d32 = mst.evaluate(pts, *mesh, pose=pose, dtype=np.float32, signed=False)[0]
    twin32 = float(np.max(np.abs(d32.astype(np.float64) - d64)))
    return max(4 * twin32, FLOOR), twin32


@pytest.mark.parametrize("name", ["sphere", "torus", "posed_box", "open_bowl", "blobs_mc"])
def test_kernel_against_twin(name):
    """Measured on the MI355X: the table in DESIGN.md section 3.13."""
    from sdfest_amd import mesh_to_sdf
    R = 64
    mesh, pose, closed = parity_scene(name)
    sdf, tri, wind = mesh_to_sdf(gpu_mesh(mesh, pose), R, normalize=False, return_triangles=True, return_winding=True)
    assert sdf.shape == tri.shape == wind.shape == (R, R, R)
    assert sdf.dtype == torch.float32 and tri.dtype == torch.int32 and wind.dtype == torch.float32
    g, gt, gw = sdf.cpu().numpy().reshape(-1), tri.cpu().numpy().reshape(-1), wind.cpu().numpy().reshape(-1)
    assert np.isfinite(g).all() and gt.min() >= 0 and gt.max() < len(mesh[1])
    # the sample: 8192 grid points, half of them near the surface
    rng = np.random.default_rng(11)
    near = np.nonzero(np.abs(g) < 3 * (2.0 / (R - 1)))[0]
    assert len(near) >= 4096
    idx = np.concatenate([rng.choice(near, 4096, replace=False), rng.choice(R ** 3, 4096, replace=False)])
    pts = mst.grid_points(R, idx)
    d64, t64, w64, d_face = mst.evaluate(pts, *mesh, pose=pose, per_face=gt[idx])
    d32, _, w32 = mst.evaluate(pts, *mesh, pose=pose, dtype=np.float32)
    twin32 = float(np.max(np.abs(d32.astype(np.float64) - d64)))
    tol = max(4 * twin32, FLOOR)
    kernel = float(np.max(np.abs(np.abs(g[idx]).astype(np.float64) - d64)))
    band = np.abs(w64 - 0.5) < 1e-3
    excluded = band | ~(d64 > tol)
    print(f"{name}: F={len(mesh[1])} distance kernel {kernel:.3e} / float32 twin {twin32:.3e} (tolerance {tol:.3e}); "
          f"winding kernel {np.max(np.abs(gw[idx] - w64)):.3e} / float32 twin {np.max(np.abs(w32 - w64)):.3e}; "
          f"excluded {100 * excluded.mean():.3f} % (winding band {100 * band.mean():.3f} %)")
    assert kernel <= tol
    assert excluded.mean() <= 0.005
    assert (band.sum() == 0) if closed else (band.mean() < 1e-3)
    assert np.array_equal((g[idx] < 0)[~excluded], (w64 > 0.5)[~excluded])
    # the reported face is a face at the minimum distance
    assert np.all(np.abs(d_face - d64) <= tol)


def separation_grids():
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    noise = np.random.default_rng(7).uniform(-1.0, 1.0, (32, 32, 32)).astype(np.float32)
    return {"sphere": (offcentre_sphere(), 0.0), "blobs": (blobs(), 0.0), "mug": (d["z0_full"], 0.02),
            "noise": (noise, 0.0)}


@pytest.mark.parametrize("name", ["sphere", "blobs", "mug", "noise"])
def test_separates_the_grid_as_marching_cubes_did(name):
    """the completed marching-cubes mesh of a grid, converted back, is negative exactly where the grid lies below the
    level: axis order, index <-> coordinate map, orientation convention and the winding sum, on every case of the table
    (white noise)"""
    from sdfest_amd import mesh_to_sdf
    grid, level = separation_grids()[name]
    R = grid.shape[0]
    m = mc_mesh(grid, level, True)
    s = mesh_to_sdf(m, R, normalize=False).cpu().numpy()
    assert np.isfinite(s).all()
    off = np.abs(s) > 1e-5
    print(f"{name}: F={m.faces.shape[0]}, {100 * (1 - off.mean()):.4f} % of the grid within 1e-5 of the surface")
    assert (~off).mean() <= 0.005
    assert np.array_equal((s < 0)[off], (grid < np.float32(level))[off])


def test_round_trip_of_a_true_distance_field():
    """|mesh_to_sdf(extract_mesh(g, 0)) - g| <= 3 h^2 / (8 r) + the distance tolerance: the sagitta of a chord of at
    most sqrt(3) h on a sphere of radius r"""
    from sdfest_amd import mesh_to_sdf
    R, r = 64, 0.55
    g = offcentre_sphere(R, radius=r)
    m = mc_mesh(g, 0.0, False)
    s = mesh_to_sdf(m, R, normalize=False).cpu().numpy()
    mesh = (m.vertices.cpu().numpy(), m.faces.cpu().numpy())
    idx = np.random.default_rng(5).choice(R ** 3, 2048, replace=False)
    tol, _ = distance_tolerance(mst.grid_points(R, idx), mesh, IDENTITY)
    h = 2.0 / (R - 1)
    err = float(np.max(np.abs(s.astype(np.float64) - g)))
    print(f"round trip: max |difference| {err:.3e}, bound {3 * h * h / (8 * r) + tol:.3e}")
    assert err <= 3 * h * h / (8 * r) + tol


def _bitwise_meshes():
    box_pose = (float(np.float32(0.45)), unit([0.31, -0.52, 0.2, 0.77]), (0.1, -0.05, 0.08))
    return [gpu_mesh(rt.uv_sphere(24, 32, 0.7)), gpu_mesh(rt.cube(1.0), box_pose), gpu_mesh(mst.bowl()),
            gpu_mesh(mst.torus(40, 20))]


def _all(mesh, R=32, **kw):
    from sdfest_amd import mesh_to_sdf
    return mesh_to_sdf(mesh, R, normalize=False, return_triangles=True, return_winding=True, **kw)


def _same(a, b):
    """bitwise, NaN included"""
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_batch_equals_single_calls_and_runs_repeat():
    meshes = _bitwise_meshes()
    singles = [_all(m) for m in meshes]
    batch = _all(meshes)
    assert batch[0].shape == (len(meshes), 32, 32, 32)
    for k, s in enumerate(singles):
        assert _same(s, [b[k] for b in batch]), k
    order = [2, 0, 3, 1, 2]
    shuffled = _all([meshes[k] for k in order])
    for j, k in enumerate(order):
        assert _same(singles[k], [b[j] for b in shuffled]), (j, k)
    assert _same(batch, _all(meshes))


def test_unsigned_is_the_absolute_value_bit_for_bit():
    from sdfest_amd import mesh_to_sdf
    for m in _bitwise_meshes():
        signed, tri, _ = _all(m)
        unsigned, tri_u = mesh_to_sdf(m, 32, normalize=False, signed=False, return_triangles=True)
        assert (signed < 0).any()
        assert torch.equal(unsigned.view(torch.int32), signed.abs().view(torch.int32)) and torch.equal(tri, tri_u)


def test_face_permutation_leaves_the_unsigned_field():
    from sdfest_amd import mesh_to_sdf
    v, f = mst.torus(40, 20)
    perm = np.random.default_rng(3).permutation(len(f))
    a, ta = mesh_to_sdf(gpu_mesh((v, f)), 32, normalize=False, signed=False, return_triangles=True)
    b, tb = mesh_to_sdf(gpu_mesh((v, f[perm])), 32, normalize=False, signed=False, return_triangles=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ta, tb = ta.cpu().numpy().reshape(-1), perm[tb.cpu().numpy().reshape(-1)]     # face j of the permuted mesh is perm[j]
    # the closest face is the same one, except where two faces tie bit for bit (a closest point on a shared edge or
    # vertex: the lowest index wins, and the permutation changes which that is) -- there both are at the minimum
    differ = np.nonzero(ta != tb)[0]
    print(f"permutation: {len(differ)} of {len(ta)} points name another face of equal distance")
    if len(differ):
        pts = mst.grid_points(32, differ)
        d64, _, _, da = mst.evaluate(pts, v, f, signed=False, per_face=ta[differ])
        db = mst.evaluate(pts, v, f, signed=False, per_face=tb[differ])[3]
        tol, _ = distance_tolerance(pts, (v, f), IDENTITY)
        assert np.all(np.abs(da - d64) <= tol) and np.all(np.abs(db - d64) <= tol)


def test_invalid_triangles_change_no_bit():
    v, f = mst.torus(40, 20)
    V = len(v)
    # three points on a line (zero area) and a NaN vertex behind the mesh's own
    v2 = np.concatenate([v, [[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.4, 0.4, 0.4], [np.nan, 0.0, 0.0]]]).astype(np.float32)
    bad = np.array([[V, V + 1, V + 2], [5, 5, 9], [3, 7, 3], [1, 2, V + 4], [1, -1, 2], [0, 1, V + 3],
                    [4, 2 ** 31 - 1, 6]], dtype=np.int32)
    ref = _all(gpu_mesh((v, f)))
    got = _all(gpu_mesh((v2, np.concatenate([f, bad]))))
    assert _same(ref, got)
    mixed = np.concatenate([bad[:3], f[:800], bad[3:], f[800:]])
    got = _all(gpu_mesh((v2, mixed)))     # the valid faces keep their order: the same sums, the faces renumbered
    assert _same([ref[0], ref[2]], [got[0], got[2]])
    renumbered = got[1] - torch.where(got[1] >= 803, 7, 3)
    assert torch.equal(ref[1], renumbered.to(torch.int32))
    # only invalid faces: NaN and -1, alone and inside a batch (the neighbours are untouched)
    sdf, tri, wind = _all(gpu_mesh((v2, bad)))
    assert torch.isnan(sdf).all() and torch.isnan(wind).all() and (tri == -1).all()
    batch = _all([gpu_mesh((v, f)), gpu_mesh((v2, bad)), gpu_mesh((v, f))])
    assert torch.isnan(batch[0][1]).all() and (batch[1][1] == -1).all()
    assert _same(ref, [b[0] for b in batch]) and _same(ref, [b[2] for b in batch])


def test_captured_graph_replay_equals_eager():
    from sdfest_amd import _lib, sdf_utils
    meshes = _bitwise_meshes()[:3]
    R, K = 32, 3
    table, total, max_f, keep = sdf_utils._mesh_sdf_table(meshes, False, R, 0)
    ws = torch.empty(_lib.lib().sdfr_mesh_sdf_workspace_bytes(K, total, max_f, R), dtype=torch.uint8, device="cuda")
    eager = [torch.empty((K, R, R, R), device="cuda"), torch.empty((K, R, R, R), dtype=torch.int32, device="cuda"),
             torch.empty((K, R, R, R), device="cuda")]
    sdf_utils._mesh_sdf_launch(table, total, max_f, 0, *eager, workspace=ws)
    torch.cuda.synchronize()
    out = [torch.full_like(t, 7) for t in eager]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            sdf_utils._mesh_sdf_launch(table, total, max_f, 0, *out, workspace=ws)
    for t in out:
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(eager, out)
    del keep


def test_normalised_framing():
    from sdfest_amd import mesh_to_sdf
    R, p = 32, 2
    lim = (R - 2 * p) / R
    # a box, longest along x, far from the origin and at another scale
    v, f = rt.cube(1.0)
    v = (v * np.array([1.0, 0.6, 0.5], dtype=np.float32) * 3.7 + np.array([5.0, -2.0, 1.0], dtype=np.float32))
    for mesh in ((v.astype(np.float32), f), tuple(a * b for a, b in zip(mst.torus(40, 20), (2.5, 1)))):
        vv = mesh[0].astype(np.float64)
        lo, hi = vv.min(0), vv.max(0)
        host = ((vv - (lo + hi) / 2) * (2.0 / (hi - lo).max()) * lim).astype(np.float32)
        a = mesh_to_sdf(gpu_mesh(mesh), R, padding=p)
        b = mesh_to_sdf(gpu_mesh((host, mesh[1])), R, normalize=False)
        err = float((a - b).abs().max())
        print(f"normalize=True against a host-normalised copy: {err:.2e}")
        assert err <= 1e-6
        # scale and pose of the mesh do not enter the normalised framing
        posed = gpu_mesh(mesh, (0.3, unit([0.1, 0.2, 0.3, 0.9]), (0.2, 0.1, -0.3)))
        assert torch.equal(mesh_to_sdf(posed, R, padding=p), a)
    # the box: along its longest axis the zero level set reaches (R - 2 p) / R and no further
    a = mesh_to_sdf(gpu_mesh((v.astype(np.float32), f)), R, padding=p).cpu().numpy()
    x = mst.grid_axis(R).astype(np.float64)
    line = a[:, R // 2, R // 2]
    clear = np.abs(np.abs(x) - lim) > 1e-5
    assert clear.sum() >= R - 2
    assert np.array_equal((line < 0)[clear], (np.abs(x) < lim)[clear])
    assert (line < 0).any() and (line > 0).any()


@pytest.fixture(scope="module")
def vae():
    import encoder_twin as et
    import test_decoder_gpu as D
    from sdfest_amd import SDFVAE
    g = np.load(os.path.join(GOLDEN, "encoder_mug.npz"))
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    w = np.load(os.path.join(GOLDEN, "mug_decoder_weights.npz"))
    state = {k: w[k] for k in w.files}
    state.update({k: g[k] for k in g.files if k.startswith("encoder.")})
    cfg = D.mug_config(d)
    cfg["encoder"] = et.MUG_ENCODER
    return SDFVAE.from_config(cfg, state)


def test_vae_reconstruction_is_its_composition(vae):
    from sdfest_amd import evaluate_metrics, extract_mesh, mesh_to_sdf, sample_points, vae_reconstruction
    from sdfest_amd.evaluation import DEFAULT_METRICS
    from sdfest_amd.sdf_utils import normalized_mesh
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    gt = mc_mesh(d["z0_full"], 0.02, True)
    gt.update_scale(0.13, rel_scale=True)           # neither scale nor pose enters
    gt.position = T([0.3, 0.1, -0.7])
    samples, seed, level, pad = 10000, 4, 0.02, 2
    metrics, latent, details = vae_reconstruction(vae, gt, samples, seed, None, level, 64, pad, return_details=True)
    again, latent2 = vae_reconstruction(vae, gt, samples, seed, level=level, padding=pad)
    assert metrics == again and torch.equal(latent, latent2) and latent.shape == (1, 8)
    with torch.no_grad():
        x = mesh_to_sdf(gt, 64, pad).view(1, 1, 64, 64, 64)
        assert torch.equal(x[0, 0], details["sdf"])
        vae.prepare_input(x)
        means, _ = vae.encoder(x)
        recon = vae.decode(means)
        mesh = extract_mesh(recon[0, 0], level, complete=True)
    a = sample_points([normalized_mesh(gt, 64, pad)], samples, seed)[0]
    b = sample_points([mesh], samples, seed)[0]
    by_hand = evaluate_metrics(a, b, DEFAULT_METRICS)
    assert torch.equal(means, latent) and torch.equal(a, details["gt_points"]) and torch.equal(b, details["points"])
    assert by_hand == metrics
    print("vae_reconstruction of the mug's own mesh:", metrics)
    assert set(metrics) == set(DEFAULT_METRICS) and all(np.isfinite(v) for v in metrics.values())


def test_process_meshes_tool(tmp_path, capsys):
    from sdfest_amd import Mesh, mesh_to_sdf
    spec = importlib.util.spec_from_file_location("process_meshes", os.path.join(ROOT, "tools", "process_meshes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src, dst = tmp_path / "in", tmp_path / "out"
    (src / "sub").mkdir(parents=True)
    gpu_mesh(mst.torus(40, 20)).write_obj(str(src / "b_torus.obj"))
    gpu_mesh(mst.bowl()).write_ply(str(src / "sub" / "a_bowl.ply"))
    (src / "notes.txt").write_text("not a mesh")
    R, p = 24, 1
    assert tool.main(["--inpath", str(src), "--outpath", str(dst), "--resolution", str(R), "--padding", str(p),
                      "--batch", "2"]) == 0
    rows = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert [r["path"] for r in rows] == ["b_torus.obj", os.path.join("sub", "a_bowl.ply")]
    assert [r["file"] for r in rows] == ["00000.npy", "00001.npy"] and [r["faces"] for r in rows] == [1600, 408]
    assert rows[0]["uncertain_share"] == 0.0 and rows[1]["uncertain_share"] > 0.01    # closed / open
    assert sorted(os.listdir(dst)) == ["00000.npy", "00001.npy"]
    for row in rows:
        vol = np.load(dst / row["file"])
        assert vol.dtype == np.float32 and vol.shape == (R, R, R)
        direct = mesh_to_sdf(Mesh.from_file(str(src / row["path"])), R, p).cpu().numpy()
        assert np.array_equal(vol, direct)
