"""GPU: reconstruction metrics (sdfest_amd.metrics over sdfr_nn_query / sdfr_nn_reduce) against the reference's values
(tests/golden/metrics.npz) and the numpy twin tests/metrics_twin.py; surface sampling (Mesh.sample_points_uniformly /
sample_points over sdfr_sample_points) against the twin and against its distribution; and the evaluation loop end to
end: mesh -> pose -> sample -> score."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN
import metrics_twin as mt

pytestmark = pytest.mark.gpu

P_NORMS = {"1": 1, "2": 2, "inf": np.inf, "3": 3}
# sdfest/estimation/configs/rendering_evaluation.yaml, key metrics:
RENDERING_EVALUATION = {
    "mean_accuracy": {"f": "sdfest.estimation.metrics.mean_accuracy", "kwargs": {}},
    "mean_completeness": {"f": "sdfest.estimation.metrics.mean_completeness", "kwargs": {}},
    "chamfer": {"f": "sdfest.estimation.metrics.symmetric_chamfer", "kwargs": {}},
    "completeness_0_01": {"f": "sdfest.estimation.metrics.completeness_thresh", "kwargs": {"threshold": 0.01}},
    "accuracy_0_01": {"f": "sdfest.estimation.metrics.accuracy_thresh", "kwargs": {"threshold": 0.01}},
}


@pytest.fixture(scope="module")
def G():
    d = np.load(os.path.join(GOLDEN, "metrics.npz"))
    return {k: d[k] for k in d.files}


def rel_close(a, b, rel=1e-6):
    a, b = float(a), float(b)
    if not np.isfinite(b):
        return a == b
    return abs(a - b) <= rel * abs(b) + 1e-12


def bits(t):
    return t.cpu().numpy().view(np.uint64) if t.dtype == torch.float64 else t.cpu().numpy()


@pytest.mark.parametrize("p", list(P_NORMS))
def test_every_metric_matches_the_reference(G, p):
    from sdfest_amd import metrics as M
    for case in G["case_names"]:
        gt_np, rec_np = G[f"{case}/gt"], G[f"{case}/rec"]
        gt, rec = torch.tensor(gt_np, device="cuda"), rec_np   # a CUDA tensor and a numpy array
        for nz, ts in ((0, G[f"{case}/t_raw"]), (1, G[f"{case}/t_norm"])):
            key, kw = f"{case}/p{p}/n{nz}", dict(p_norm=P_NORMS[p], normalize=bool(nz))
            for name in ("mean_accuracy", "mean_completeness", "symmetric_chamfer"):
                got = getattr(M, name)(gt, rec, **kw)
                assert isinstance(got, float) and rel_close(got, G[f"{key}/{name}"]), (key, name, got)
            for name in ("accuracy_thresh", "completeness_thresh", "reconstruction_fscore"):
                got = [getattr(M, name)(gt, rec, float(t), **kw) for t in ts]
                assert got == G[f"{key}/{name}"].tolist(), (key, name, got)
        assert rel_close(M.extent(gt_np), G[f"{case}/extent"])


def test_fscore_zero_is_the_int_and_correct_thresh_fscore(G):
    from sdfest_amd import metrics as M
    gt = np.zeros((5, 3), np.float32)
    far = np.full((7, 3), 1.0, np.float32)
    got = M.reconstruction_fscore(gt, far, 0.01)
    assert got == 0 and type(got) is int
    gt, rec = G["sphere/gt"], G["sphere/rec"]
    for t, want in zip(G["correct/fscore_thresholds"], G["correct/fscore_result"]):
        assert M.correct_thresh(np.zeros(3), np.zeros(3), [0, 0, 0, 1], [0, 0, 0, 1], points_gt=gt,
                                points_prediction=rec, fscore_threshold=float(t)) == want


def test_empty_or_nonfinite_sets_raise():
    from sdfest_amd import metrics as M
    x = np.random.default_rng(0).normal(size=(10, 3)).astype(np.float32)
    with pytest.raises(ValueError):
        M.mean_accuracy(x, np.zeros((0, 3), np.float32))
    bad = x.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        M.mean_completeness(x, bad)
    bad[3, 1] = np.inf
    with pytest.raises(ValueError):
        M.symmetric_chamfer(torch.tensor(bad, device="cuda"), x)


@pytest.mark.parametrize("p", [1, 2, np.inf])
def test_nearest_indices_equal_the_twin_with_ties_at_the_lowest_index(G, p):
    from sdfest_amd.metrics import nearest_neighbors
    gt, rec = G["ties/gt"], G["ties/rec"]
    for q, r in ((rec, gt), (gt, rec), (G["sphere/rec"], G["sphere/gt"])):
        d, i = nearest_neighbors(q, r, p_norm=p)
        td, ti = mt.nearest(q, r, p)
        assert np.array_equal(i.cpu().numpy(), ti)
        assert np.array_equal(d.cpu().numpy(), td)
        d, i = nearest_neighbors(q, r, p_norm=p, farthest=True)
        td, ti = mt.nearest(q, r, p, farthest=True)
        assert np.array_equal(i.cpu().numpy(), ti)
        assert np.array_equal(d.cpu().numpy(), td)


@pytest.mark.parametrize("nq,nr", [(1, 1), (63, 65), (64, 64), (65, 63), (4097, 65), (65, 4097), (1, 100000),
                                   (100000, 1)])
def test_sizes_off_the_tile(nq, nr):
    from sdfest_amd.metrics import nearest_neighbors
    rng = np.random.default_rng(nq * 7 + nr)
    q = rng.uniform(-1, 1, (nq, 3)).astype(np.float32)
    r = rng.uniform(-1, 1, (nr, 3)).astype(np.float32)
    for p in (2, 1):
        d, i = nearest_neighbors(q, r, p_norm=p)
        td, ti = mt.nearest(q, r, p, chunk=max(1, 4000000 // nr))
        assert np.array_equal(i.cpu().numpy(), ti) and np.array_equal(d.cpu().numpy(), td), (nq, nr, p)


def test_ragged_batch_equals_single_calls_and_runs_repeat(G):
    from sdfest_amd import metrics as M
    rng = np.random.default_rng(4)
    gts = [G["sphere/gt"], G["hand/gt"], rng.normal(size=(1500, 3)).astype(np.float32) * 0.1, G["ties/gt"]]
    recs = [G["sphere/rec"], G["hand/rec"], rng.normal(size=(333, 3)).astype(np.float32) * 0.1, G["ties/rec"]]
    ths = (0.01, 0.1, 0.2, 0.004, 0.05)   # more than one reduce launch (4 thresholds each)
    for normalize in (False, True):
        for p in (2, 3):
            batch = M.reconstruction_metrics(gts, recs, thresholds=ths, p_norm=p, normalize=normalize)
            again = M.reconstruction_metrics(gts, recs, thresholds=ths, p_norm=p, normalize=normalize)
            assert batch.keys() == again.keys()
            for k in batch:
                assert batch[k].shape == (4,) and batch[k].dtype == torch.float64
                assert np.array_equal(bits(batch[k]), bits(again[k])), k
            for j, (g, r) in enumerate(zip(gts, recs)):
                kw = dict(p_norm=p, normalize=normalize)
                assert batch["accuracy"][j].item() == M.mean_accuracy(g, r, **kw)
                assert batch["completeness"][j].item() == M.mean_completeness(g, r, **kw)
                assert batch["chamfer"][j].item() == M.symmetric_chamfer(g, r, **kw)
                for t in ths:
                    assert batch[f"accuracy@{t:g}"][j].item() == M.accuracy_thresh(g, r, t, **kw)
                    assert batch[f"completeness@{t:g}"][j].item() == M.completeness_thresh(g, r, t, **kw)
                    assert batch[f"fscore@{t:g}"][j].item() == M.reconstruction_fscore(g, r, t, **kw)
                if normalize:
                    assert batch["extent"][j].item() == M.extent(g)
    # a dense (K, N, 3) batch is the same as its list
    a = torch.tensor(np.stack([gts[2][:300], gts[2][300:600]]), device="cuda")
    b = torch.tensor(np.stack([recs[2][:100], recs[2][100:200]]), device="cuda")
    dense = M.reconstruction_metrics(a, b)
    listed = M.reconstruction_metrics(list(a), list(b))
    assert all(np.array_equal(bits(dense[k]), bits(listed[k])) for k in dense)


def test_extent_is_the_diameter():
    from sdfest_amd import metrics as M
    x = np.random.default_rng(9).normal(size=(3000, 3)).astype(np.float32) * np.float32([1.0, 0.3, 0.1])
    x64 = x.astype(np.float64)
    diam = max(np.sqrt(((x64[s:s + 500, None] - x64[None]) ** 2).sum(-1)).max() for s in range(0, len(x), 500))
    assert rel_close(M.extent(torch.tensor(x, device="cuda")), diam)
    assert M.extent(x[:1]) == 0.0


def test_evaluate_metrics_equals_the_individual_calls(G):
    from sdfest_amd import metrics as M
    gt, rec = G["sphere/gt"], G["sphere/rec"]
    got = M.evaluate_metrics(gt, rec, RENDERING_EVALUATION)
    assert list(got) == list(RENDERING_EVALUATION)
    assert got["mean_accuracy"] == M.mean_accuracy(gt, rec)
    assert got["mean_completeness"] == M.mean_completeness(gt, rec)
    assert got["chamfer"] == M.symmetric_chamfer(gt, rec)
    assert got["completeness_0_01"] == M.completeness_thresh(gt, rec, 0.01)
    assert got["accuracy_0_01"] == M.accuracy_thresh(gt, rec, 0.01)
    # normalised and p-norm entries share passes too (redwood_evaluation.yaml style)
    cfg = {"norm_acc": {"f": "sdfest.estimation.metrics.mean_accuracy", "kwargs": {"normalize": True}},
           "norm_c_0_1": {"f": "sdfest.estimation.metrics.completeness_thresh",
                          "kwargs": {"threshold": 0.05, "normalize": True}},
           "f_l1": {"f": "sdfest.estimation.metrics.reconstruction_fscore", "kwargs": {"threshold": 0.01, "p_norm": 1}}}
    got = M.evaluate_metrics(gt, rec, cfg)
    assert got["norm_acc"] == M.mean_accuracy(gt, rec, normalize=True)
    assert got["norm_c_0_1"] == M.completeness_thresh(gt, rec, 0.05, normalize=True)
    assert got["f_l1"] == M.reconstruction_fscore(gt, rec, 0.01, p_norm=1)


# ---- sampling -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mug():
    from sdfest_amd import extract_mesh
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    return extract_mesh(torch.tensor(d["z0_full"], device="cuda"), 0.02, normals=True)


def posed(mesh, q, p, scale):
    from sdfest_amd import Mesh
    m = Mesh(mesh.vertices, mesh.faces, mesh.normals, scale=scale, rel_scale=True)
    m.orientation, m.position = q, p
    return m


Q = np.array([0.2, -0.4, 0.1, 0.9], np.float32) / np.float32(np.linalg.norm([0.2, -0.4, 0.1, 0.9]))
P = np.array([0.05, -0.1, 0.7], np.float32)


def test_sampling_repeats_and_batches_bit_for_bit(mug):
    from sdfest_amd import extract_mesh, sample_points
    from sdfest_amd.synthetic import sphere_sdf
    a = posed(mug, Q, P, 0.1)
    b = extract_mesh(torch.tensor(sphere_sdf(0.4, 32), device="cuda"), 0.0)
    c = posed(mug, [0, 0, 0, 1], [0, 0, 0], 2.0)
    x1 = a.sample_points_uniformly(5000, seed=3)
    x2 = a.sample_points_uniformly(5000, seed=3)
    assert torch.equal(x1.view(torch.int32), x2.view(torch.int32))
    assert not torch.equal(x1, a.sample_points_uniformly(5000, seed=4))
    batch = sample_points([b, a, c], 5000, seed=3)
    assert batch.shape == (3, 5000, 3)
    assert torch.equal(batch[1].view(torch.int32), x1.view(torch.int32))
    assert torch.equal(batch[0].view(torch.int32), b.sample_points_uniformly(5000, seed=3).view(torch.int32))
    assert torch.equal(batch[2].view(torch.int32), c.sample_points_uniformly(5000, seed=3).view(torch.int32))


def test_sampling_equals_the_twin(mug):
    m = posed(mug, Q, P, 0.1)
    pts, tri = m.sample_points_uniformly(20000, seed=11, return_triangles=True)
    want, wt, margin = mt.sample_points(mug.vertices.cpu().numpy(), mug.faces.cpu().numpy(), 20000, 11,
                                        factor=m._factor, quat=Q, position=P)
    tri = tri.cpu().numpy()
    same = tri == wt
    assert np.all(same | (margin < 1e-9)), np.flatnonzero(~same)[:5]
    assert same.mean() > 0.999
    assert np.abs(pts.cpu().numpy()[same] - want[same]).max() <= 1e-6


def test_samples_lie_on_their_triangles(mug):
    pts, tri = mug.sample_points_uniformly(20000, seed=2, transformed=False, return_triangles=True)
    v = mug.vertices.double().cpu().numpy()
    f = mug.faces.cpu().numpy()[tri.cpu().numpy()]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    x = pts.double().cpu().numpy()
    n = np.cross(b - a, c - a)
    nn = np.linalg.norm(n, axis=1)
    assert np.all(nn > 0)                                         # zero-area faces are never chosen
    assert np.abs(((x - a) * n).sum(1) / nn).max() < 1e-6         # on the plane
    # barycentric coordinates from the point: all >= 0 (to rounding)
    e0, e1, e2 = b - a, c - a, x - a
    d00, d01, d11 = (e0 * e0).sum(1), (e0 * e1).sum(1), (e1 * e1).sum(1)
    d20, d21 = (e2 * e0).sum(1), (e2 * e1).sum(1)
    den = d00 * d11 - d01 * d01
    wb = (d11 * d20 - d01 * d21) / den
    wc = (d00 * d21 - d01 * d20) / den
    assert min(wb.min(), wc.min(), (1 - wb - wc).min()) > -1e-4


def test_triangle_hits_follow_the_areas(mug):
    n = 200000
    _, tri = mug.sample_points_uniformly(n, seed=5, transformed=False, return_triangles=True)
    area = mt.face_areas(mug.vertices.cpu().numpy(), mug.faces.cpu().numpy())
    e = n * area / area.sum()
    h = np.bincount(tri.cpu().numpy(), minlength=len(area))
    assert h[area == 0].sum() == 0
    live = e > 0
    chi2 = np.sum((h[live] - e[live]) ** 2 / e[live])
    dof = live.sum() - 1
    assert abs(chi2 - dof) < 5 * np.sqrt(2 * dof), (chi2, dof)


def test_transformed_is_the_posed_untransformed(mug):
    from sdfest_amd.pipeline import quaternion_apply
    m = posed(mug, Q, P, 0.1)
    x, nx = m.sample_points_uniformly(4000, seed=8, normals=True)
    y, ny = m.sample_points_uniformly(4000, seed=8, transformed=False, normals=True)
    q = torch.tensor(Q, device="cuda").expand(4000, 4)
    assert (quaternion_apply(q, y) + torch.tensor(P, device="cuda") - x).abs().max().item() < 1e-6
    assert (quaternion_apply(q, ny) - nx).abs().max().item() < 1e-5
    assert (nx.norm(dim=1) - 1).abs().max().item() < 1e-5


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_mug_scored_against_itself():
    from sdfest_amd import metrics as M
    from test_mesh_gpu import make_pipeline
    pipe, _ = make_pipeline()
    z = torch.tensor(np.load(os.path.join(GOLDEN, "decoder_mug.npz"))["z"][:1], device="cuda")
    mesh = pipe.generate_mesh(z, torch.tensor([0.1], device="cuda"), complete_mesh=True)
    mesh.position, mesh.orientation = P, Q
    n = 20000
    a = mesh.sample_points_uniformly(n, seed=0)
    b = mesh.sample_points_uniformly(n, seed=1)
    area = mt.face_areas(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()).sum() / 2 * mesh._factor ** 2
    chamfer = M.symmetric_chamfer(a, b)
    assert chamfer < 0.75 * np.sqrt(area / n), (chamfer, area)
    assert M.reconstruction_fscore(a, b, 0.01) >= 0.999


def test_concentric_spheres_are_delta_apart():
    from sdfest_amd import extract_mesh, metrics as M
    from sdfest_amd.synthetic import sphere_sdf
    delta = 0.1
    grid = torch.tensor(sphere_sdf(0.5, 64), device="cuda")
    inner, outer = extract_mesh(torch.stack([grid, grid]), 0.0)[0], extract_mesh(grid, delta)
    a = inner.sample_points_uniformly(20000, seed=0)
    b = outer.sample_points_uniformly(20000, seed=1)
    assert abs(M.mean_accuracy(a, b) - delta) < 0.05 * delta
    assert abs(M.mean_completeness(a, b) - delta) < 0.05 * delta
