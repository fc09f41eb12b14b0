"""GPU: sdfr_similarity_ransac (sdfest_amd/csrc/nocs.hip) on the edge cases of tests/nocs_edges.py, which
tests/test_nocs_edges_cpu.py shows to be what they were built to be.

Directed cases and the sweep are compared with tests/nocs_twin.py on the same draws: status, iterations run, winner,
inlier mask and inlier ratio exactly; position, rotation, scale and transform to 1e-10 * max(1, max|twin value|) per
array -- tests/test_nocs_gpu.py's ATOL, the bound of the reference's own test, relative to the array's magnitude so that
the fit at scale 1e3 is measured by its own size.  A winner is compared as a HYPOTHESIS: rows that sample the same five
points in another order differ by rounding only (every row of a 5-point set, most rows of a 6-point set), so the
kernel's winner must sample the twin's winner's points, and is the same row whenever that point set was drawn once.

The degenerate families (exactly planar and exactly collinear sources) have no single answer: a rotation and its mirror
image fit them equally well, and which of the two the reference returns is decided by rounding.  There the kernel must
return a ROTATION that is one of the minimisers, and the twin's scale (which does not depend on the side)."""
import json
import os

import numpy as np
import pytest
import torch

import nocs_edges as ne
import nocs_twin as tw
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

RTOL = 1e-10
OUTPUTS = (("position", "position"), ("rotation_matrix", "rotation"), ("scale", "scale"), ("transform", "transform"))
RESULTS = ("position", "rotation_matrix", "scale", "transform", "inlier_ratio", "status", "best_iteration",
           "iterations_run")

with open(os.path.join(GOLDEN, ne.SEEDS_FILE)) as f:
    SEEDS = json.load(f)
DIRECTED = ne.directed_cases(SEEDS)
SWEEP = ne.sweep_cases(SEEDS)
DEGENERATE = ne.degenerate_families()
FAMILIES = ("mirrored", "symmetric", "aligned", "scale", "nan", "pose_error")
_twin = {}


def twin(key, c):
    """the twin's result of a case, computed once"""
    if key not in _twin:
        _twin[key] = tw.ransac(c["source"], c["target"], c["draws"])
    return _twin[key]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def run(cases, dev):
    """one call over the cases (all of one dtype) as the K objects of a batch; host copies of every result"""
    from sdfest_amd import nocs_utils as nu
    src = np.concatenate([c["source"] for c in cases])
    tgt = np.concatenate([c["target"] for c in cases])
    assert src.dtype == tgt.dtype and all(c["source"].dtype == src.dtype == c["target"].dtype for c in cases)
    offsets = np.concatenate([[0], np.cumsum([len(c["source"]) for c in cases])]).tolist()
    draws = torch.tensor(np.stack([c["draws"] for c in cases]), dtype=torch.int32, device=dev)
    r = nu.estimate_similarity_transforms(torch.tensor(src, device=dev), torch.tensor(tgt, device=dev), offsets,
                                          sample_indices=draws, with_inlier_mask=True)
    torch.cuda.synchronize()
    host = {k: getattr(r, k).cpu().numpy() for k in r._fields}
    host["offsets"] = offsets
    return host


def run_by_dtype(named, dev):
    """{name: (host results, k)}: one call per dtype over the named cases of that dtype"""
    out = {}
    for dtype in (np.float32, np.float64):
        names = [n for n, c in named.items() if c["source"].dtype == dtype]
        if names:
            h = run([named[n] for n in names], dev)
            out.update({n: (h, k) for k, n in enumerate(names)})
    return out


def check_against_twin(name, c, o, h, k):
    """every choice exactly, every output within RTOL of its array's magnitude; returns the largest error over bound"""
    a, b = h["offsets"][k], h["offsets"][k + 1]
    assert h["status"][k] == o["status"], name
    assert h["iterations_run"][k] == o["iterations_run"], name
    assert ne.same_hypothesis(c, int(h["best_iteration"][k]), o["best_iteration"]), name
    assert np.array_equal(np.nonzero(h["inlier_mask"][a:b])[0], o["inlier_idx"]), name
    assert set(np.unique(h["inlier_mask"][a:b])) <= {0, 1}, name
    assert h["inlier_ratio"][k] == o["inlier_ratio"], name
    if o["status"] != tw.OK:
        for ours, _ in OUTPUTS:
            assert np.all(np.isnan(h[ours][k])), (name, ours)
        return 0.0
    worst = 0.0
    for ours, key in OUTPUTS:
        want = np.asarray(o[key], np.float64)
        err = np.max(np.abs(h[ours][k] - want)) / max(1.0, np.max(np.abs(want)))
        assert err <= RTOL, (name, key, err)
        worst = max(worst, err)
    return worst


@pytest.mark.parametrize("family", FAMILIES)
def test_directed_family_equals_the_twin(family, dev):
    named = {n: c for n, c in DIRECTED.items() if c["family"] == family}
    worst = {}
    failures = []
    for name, (h, k) in run_by_dtype(named, dev).items():
        try:
            worst[name] = check_against_twin(name, named[name], twin(name, named[name]), h, k)
        except AssertionError as e:
            failures.append(str(e).splitlines()[0])
    print(f"{family}: largest error / max(1, max|twin|) {max(worst.values(), default=0.0):.3e} over {len(worst)} of "
          f"{len(named)} cases")
    assert not failures, failures


@pytest.fixture(scope="module")
def sweep_batched(dev):
    return run_by_dtype(SWEEP, dev)


def test_sweep_equals_the_twin(sweep_batched):
    worst = {}
    failures = []
    for name, (h, k) in sweep_batched.items():
        try:
            worst[name] = check_against_twin(name, SWEEP[name], twin(name, SWEEP[name]), h, k)
        except AssertionError as e:
            failures.append(str(e).splitlines()[0])
    print(f"sweep: largest error / max(1, max|twin|) {max(worst.values(), default=0.0):.3e} over {len(worst)} of "
          f"{len(SWEEP)} cases")
    assert len(sweep_batched) == ne.SWEEP_SLOTS and not failures, failures


def test_each_sweep_object_alone_equals_its_batched_result_bit_for_bit(dev, sweep_batched):
    for name, (h, k) in sweep_batched.items():
        single = run([SWEEP[name]], dev)
        for key in RESULTS:
            assert single[key][0].tobytes() == h[key][k].tobytes(), (name, key)
        a, b = h["offsets"][k], h["offsets"][k + 1]
        assert np.array_equal(single["inlier_mask"], h["inlier_mask"][a:b]), name


def rms_residual(scale, R, position, src, tgt):
    return np.sqrt(np.mean(np.sum((tgt - (scale * src @ R.T + position)) ** 2, axis=1)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("family", sorted(DEGENERATE))
def test_degenerate_family_gets_a_rotation_that_minimises(family, dtype, dev):
    """every object: status OK, R orthogonal to 1e-12 with det R > 0, the twin's scale to 1e-10 relative, and an RMS
    residual over the inliers (all points) of at most the twin's + 1e-12 * max(1, max|target|).  R and position are
    not compared with the twin: they legitimately differ between minimisers."""
    cases = [dict(c, source=c["source"].astype(dtype), target=c["target"].astype(dtype)) for c in DEGENERATE[family]]
    h = run(cases, dev)
    rows = []
    for k, c in enumerate(cases):
        o = twin((family, np.dtype(dtype).name, k), c)
        src, tgt = c["source"].astype(np.float64), c["target"].astype(np.float64)
        assert o["status"] == tw.OK and len(o["inlier_idx"]) == len(src)
        R, a, b = h["rotation_matrix"][k], h["offsets"][k], h["offsets"][k + 1]
        ok = h["status"][k] == tw.OK and bool(np.all(h["inlier_mask"][a:b] == 1))
        ortho = np.max(np.sum(np.abs(R.T @ R - np.eye(3)), axis=1))
        excess = (rms_residual(h["scale"][k], R, h["position"][k], src, tgt)
                  - rms_residual(o["scale"], o["rotation"], o["position"], src, tgt)) / max(1.0, np.max(np.abs(tgt)))
        rows.append((ok, ortho, np.linalg.det(R), abs(h["scale"][k] / o["scale"] - 1), excess,
                     np.linalg.det(o["rotation"])))
    ok, ortho, det, scale_err, excess, twin_det = (np.array(v) for v in zip(*rows))
    print(f"{family} {np.dtype(dtype).name}: status OK over all points {int(ok.sum())}/{len(rows)}, det R < 0 in "
          f"{int(np.sum(det < 0))} (twin: {int(np.sum(twin_det < 0))}), largest |R^T R - I| {ortho.max():.3e}, scale "
          f"error {scale_err.max():.3e}, residual above the twin's {excess.max():.3e}")
    assert ok.all()
    assert np.all(ortho <= 1e-12), ortho.max()
    assert np.all(det > 0), f"{int(np.sum(det < 0))} of {len(rows)} results are reflections"
    assert np.all(scale_err <= 1e-10), scale_err.max()
    assert np.all(excess <= 1e-12), excess.max()
