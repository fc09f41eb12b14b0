"""CPU: the edge cases of the NOCS fit (tests/nocs_edges.py) are what they were built to be -- every recorded sweep
seed still passes the margins of tools/make_nocs_goldens.py (recomputed with tests/nocs_twin.py), every directed case
takes the twin's branch it was built for, and the degenerate families are exactly planar / collinear sets that the
twin fits over all their points.  tests/test_nocs_edges_gpu.py runs the same cases through the kernel."""
import json
import os
import re

import numpy as np
import pytest

import nocs_edges as ne
import nocs_twin as tw
from helpers import GOLDEN

with open(os.path.join(GOLDEN, ne.SEEDS_FILE)) as f:
    SEEDS = json.load(f)
DIRECTED = ne.directed_cases(SEEDS)
SWEEP = ne.sweep_cases(SEEDS)
_twin = {}


def twin(name, c):
    """the twin's result of a named case, computed once"""
    if name not in _twin:
        _twin[name] = tw.ransac(c["source"], c["target"], c["draws"])
    return _twin[name]


def test_sample_rows_are_the_twins_sample_indices():
    for n, seed in ((5, 1), (6, 8), (7, 9), (40, 381), (257, 2 ** 40 + 5), (1025, 4800)):
        assert np.array_equal(ne.sample_rows(n, seed), tw.sample_indices(n, seed)), (n, seed)


def test_no_sweep_slot_is_missing():
    assert len(SEEDS["sweep"]) == ne.SWEEP_SLOTS == len(SWEEP)
    slots = [ne.sweep_slot(i) for i in range(ne.SWEEP_SLOTS)]
    assert {(s[0], s[1]) for s in slots} == {(n, d) for n in ne.SWEEP_N for d in ne.SWEEP_DTYPES}
    assert {(s[2], s[3]) for s in slots} == {(a, b) for a in ne.SWEEP_SHARES for b in ne.SWEEP_NOISES}
    for (n, dtype, _, _, first), seed, c in zip(slots, SEEDS["sweep"], SWEEP.values()):
        assert first <= seed < first + ne.SWEEP_TRIES
        assert len(c["source"]) == n and c["source"].dtype == c["target"].dtype == np.dtype(dtype)
        assert c["draws"].shape == (100, 5) and c["draws"].max() < n


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_recorded_sweep_seed_passes_every_margin(name):
    assert ne.margins(SWEEP[name], twin(name, SWEEP[name])) == []


def test_sweep_reaches_the_statuses_and_both_ends_of_the_loop():
    o = [twin(n, c) for n, c in SWEEP.items()]
    assert {r["status"] for r in o} == {tw.OK, tw.NONE, tw.POSE_ERROR}
    ran = [r["iterations_run"] for r in o]
    assert 1 in ran and 100 in ran and any(1 < r < 100 for r in ran)
    # a final fit over all points and over a part of them, at every count from 127 up
    for n in ne.SWEEP_N[3:]:
        kept = [len(r["inlier_idx"]) for r, c in zip(o, SWEEP.values()) if len(c["source"]) == n and r["status"] == tw.OK]
        assert len(kept) == 4 and max(kept) == n and min(kept) < n, n


def test_directed_cases_are_the_ones_the_tests_rely_on():
    names = [f"{kind}{tag}_{n}" for n in ne.COUNTS for kind in ("flat", "mirror") for tag in list(ne.THIN) + ["x"]]
    names += ["octahedron", "cube", "slab"] + [f"{k}_{n}" for n in ne.COUNTS for k in ("same", "double")]
    names += ["scale_1e-3", "scale_1e3", "far_f32", "nan_row0", "nan_row7", "nan_unsampled", "pose_error_5",
              "pose_error_6"]
    assert sorted(DIRECTED) == sorted(names)
    assert {c["family"] for c in DIRECTED.values()} == {"mirrored", "symmetric", "aligned", "scale", "nan", "pose_error"}


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_case_takes_the_branch_it_was_built_for(name):
    c = DIRECTED[name]
    o = twin(name, c)
    n = len(c["source"])
    assert ne.margins(c, o, conditioning=False) == []
    assert o["status"] == c.get("status", tw.OK)
    if "iterations_run" in c:
        assert o["iterations_run"] == c["iterations_run"]
    if o["status"] != tw.OK:
        return
    assert abs(np.linalg.det(o["rotation"]) - 1) < 1e-12          # the twin's answer is a rotation
    cov = ne.final_covariance(c, o)
    sv = np.linalg.svd(cov, compute_uv=False)
    if c["family"] == "mirrored":
        assert len(o["inlier_idx"]) >= n - 1
        assert (np.linalg.det(cov) < 0) == (c["branch"] == "reflection")
        thickness = re.fullmatch(r"(flat|mirror)x?(\d*)_\d+", name).group(2)
        lo, hi = {"": (1e-8, 1e-6), "12": (1e-13, 1e-11), "18": (1e-19, 1e-17)}[thickness]
        assert lo < sv[2] / sv[0] < hi
    if c["family"] == "symmetric":
        assert len(o["inlier_idx"]) == n
        k = 3 if c["branch"] == "repeated" else 2
        assert np.max(np.abs(sv[:k] / sv[0] - 1)) <= 1e-12
        assert k == 3 or sv[2] < 0.5 * sv[0]
    if c["family"] == "aligned":
        assert len(o["inlier_idx"]) == n
        assert np.array_equal(cov, np.diag(np.diag(cov))) and len(set(np.diag(cov))) == 3
    if name == "scale_1e-3":
        assert abs(o["scale"] / 1e-3 - 1) < 1e-2
    if name == "scale_1e3":
        assert abs(o["scale"] / 1e3 - 1) < 1e-2
    if name == "far_f32":
        assert c["source"].dtype == c["target"].dtype == np.float32 and 29 < np.linalg.norm(o["position"]) < 31


def test_nan_and_pose_error_cases():
    c = DIRECTED["nan_row0"]
    assert np.isnan(c["source"][c["draws"][0]]).any()
    c = DIRECTED["nan_row7"]
    bad = np.nonzero(np.isnan(c["target"]).any(1))[0]
    assert len(bad) == 1 and bad[0] in c["draws"][7] and bad[0] not in c["draws"][:7]
    c = DIRECTED["nan_unsampled"]
    bad = np.nonzero(np.isnan(c["source"]).any(1))[0]
    assert len(bad) == 1 and bad[0] not in c["draws"]
    o = twin("nan_unsampled", c)
    assert o["best_iteration"] == -1 and o["inlier_ratio"] == 0.0
    assert np.array_equal(o["inlier_idx"], np.arange(len(c["source"])))
    for n in (5, 6):
        o = twin(f"pose_error_{n}", DIRECTED[f"pose_error_{n}"])
        assert o["best_iteration"] >= 0 and len(o["inlier_idx"]) == 1 and o["inlier_idx"][0] != 0


def test_degenerate_families_are_exactly_rank_deficient():
    families = ne.degenerate_families()
    assert sorted(families) == sorted(f"{k}_{n}_{e}" for k in ("planar", "collinear") for n in (5, 200)
                                      for e in ("exact", "noisy"))
    for name, cases in families.items():
        assert len(cases) == ne.DEGENERATE_SEEDS
        for c in cases:
            src = c["source"]
            assert len(src) == int(name.split("_")[1])
            k = np.round((src + 0.5) * 255)
            assert np.array_equal(src, (k.astype(np.float32) / np.float32(255) - np.float32(0.5)).astype(np.float64))
            constant = int(np.sum(np.all(src == src[0], axis=0)))
            assert constant == (1 if name.startswith("planar") else 2)
            o = tw.ransac(src, c["target"], c["draws"])
            assert o["status"] == tw.OK and len(o["inlier_idx"]) == len(src)      # the final fit is over all points
            sv = np.linalg.svd(ne.final_covariance(c, o), compute_uv=False)
            assert sv[3 - constant] <= 1e-14 * sv[0] < sv[0] * 1e-3 < sv[2 - constant]
