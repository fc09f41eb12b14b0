"""GPU: detection matching and average precision (csrc/ap.hip, sdfest_amd/ap.py) against the numpy twin
(tests/ap_twin.py): sdfr_ap_match byte for byte, sdfr_ap_integrate within 1e-12 (a sum of at most 4 096 terms in [0, 1]
and one division in fp64: N 2^-53 = 4.5e-13 bounds the difference between two summation orders), sdfr_pose_pair_errors
within 1e-12 degrees (a handful of fp64 operations on values <= 180) and 4 ulp of the distance, mean_average_precision
end to end on a small scene, and tools/evaluate_detections.py in a child process."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import ap_twin as twin
import box_iou_twin
from helpers import ROOT

pytestmark = pytest.mark.gpu

INF = float("inf")
DEV = "cuda:0"


def _lib():
    from sdfest_amd import _lib
    return _lib


def dev(a, dtype):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


# ---- sdfr_ap_match --------------------------------------------------------------------------------------------------
GROUP_SHAPES = [(0, 3), (3, 0), (1, 1), (5, 2), (2, 5), (7, 33), (3, 64)]   # detections x ground truths
PAD = 64          # bytes behind matched [T][P] that no call may touch
FILL = 0xAA


def make_groups(shapes, seed):
    """tables whose entries are multiples of 1/4 (equal keys and values ON a threshold do occur), one NaN entry"""
    rng = np.random.default_rng(seed)
    tables = []
    for nd, ng in shapes:
        t = np.stack([rng.integers(0, 5, (nd, ng)) / 4.0, rng.integers(0, 9, (nd, ng)) / 4.0,
                      rng.integers(0, 5, (nd, ng)) / 4.0, rng.integers(-4, 5, (nd, ng)) / 4.0], -1)
        tables.append(t)
    tables[3][2, 1, 1] = np.nan
    if len(tables) > 5 and tables[5].shape[1] > 32:   # ground truth 32 is everybody's first choice: bit 32 of the mask decides
        tables[5][:2, 32] = (1.0, 0.0, 0.0, -2.0)
    return tables


def pack(tables):
    nd = np.array([t.shape[0] for t in tables])
    ng = np.array([t.shape[1] for t in tables])
    off = lambda c: np.concatenate([[0], np.cumsum(c)])
    flat = np.concatenate([t.reshape(-1, 4) for t in tables]) if tables else np.zeros((0, 4))
    return flat, off(nd), off(ng), off(nd * ng)


def make_criteria(T, seed):
    rng = np.random.default_rng(seed)
    c = np.stack([rng.integers(0, 5, T) / 4.0, rng.integers(0, 9, T) / 4.0, rng.integers(0, 5, T) / 4.0], 1)
    c[rng.random(T) < 0.2, 0] = -INF
    c[rng.random(T) < 0.2, 1] = INF
    c[rng.random(T) < 0.2, 2] = INF
    c[0] = (-INF, INF, INF)
    return c


def run_match(flat, pred_off, gt_off, pair_off, criteria):
    """(matched (T,P) uint8, the PAD bytes behind it, status) of one sdfr_ap_match call on FILL-ed output"""
    lib = _lib()
    P, T, G = int(pred_off[-1]), len(criteria), len(pred_off) - 1
    table = dev(flat.reshape(-1, 4), torch.float64)
    po, go, eo = dev(pred_off, torch.int32), dev(gt_off, torch.int32), dev(pair_off, torch.int64)
    crit = dev(criteria, torch.float64)
    out = torch.full((T * P + PAD,), FILL, dtype=torch.uint8, device=DEV)
    status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    lib.check(lib.lib().sdfr_ap_match(table.data_ptr(), int(flat.reshape(-1, 4).shape[0]), po.data_ptr(), go.data_ptr(),
                                      eo.data_ptr(), G, P, crit.data_ptr(), T, out.data_ptr(), status.data_ptr(), 0,
                                      torch.cuda.current_stream().cuda_stream), "sdfr_ap_match")
    h = out.cpu().numpy()
    return h[:T * P].reshape(T, P), h[T * P:], int(status.item())


@pytest.fixture(scope="module")
def match_case():
    B = _lib().ABI["SDFR_AP_CRITERIA_BLOCK"]
    tables = make_groups(GROUP_SHAPES, 1)
    criteria = make_criteria(B + 1, 2)
    flat, po, go, eo = pack(tables)
    expected, refused = twin.match(flat, po, go, eo, criteria)
    assert not refused
    return B, tables, criteria, expected


@pytest.mark.parametrize("dT", [-1, 0, 1])
def test_match_equals_the_twin_around_the_criteria_block(match_case, dT):
    B, tables, criteria, expected = match_case
    T = B + dT
    got, pad, status = run_match(*pack(tables), criteria[:T])
    assert status == 0 and np.all(pad == FILL)
    assert got.shape == expected[:T].shape and np.array_equal(got, expected[:T])
    # the cases the tables are made for do occur: ties in the key among admissible pairs, values on a threshold
    t = tables[5]
    assert any(len(set(row)) < len(row) for row in t[..., 3])
    assert np.any(t[..., 0][:, :, None] == criteria[None, None, :T, 0])
    assert np.any((got[:, -3:] >= 32) & (got[:, -3:] < 64)) and np.any(got == 63)   # both halves of the mask, its top bit
    assert np.all(got[:, 11] == 32) and not np.any(got[:, 12] == 32)   # the 33-group: the first takes 32, the second cannot


def test_match_of_a_group_alone_equals_its_columns_among_the_others(match_case):
    B, tables, criteria, expected = match_case
    col = 0
    for t in tables:
        nd = t.shape[0]
        got, pad, status = run_match(*pack([t]), criteria)
        assert status == (0 if nd else 77) and np.all(pad == FILL)     # P = 0: the call does nothing at all
        assert got.tobytes() == np.ascontiguousarray(expected[:, col:col + nd]).tobytes()
        col += nd


def test_match_refuses_a_65_ground_truth_group_and_leaves_its_neighbours(match_case):
    B, tables, criteria, expected = match_case
    rng = np.random.default_rng(3)
    big = rng.integers(0, 5, (2, 65, 4)) / 4.0
    with_big = tables[:4] + [big] + tables[4:]
    before = sum(t.shape[0] for t in tables[:4])
    got, pad, status = run_match(*pack(with_big), criteria)
    assert status == 1 and np.all(pad == FILL)
    assert np.all(got[:, before:before + 2] == twin.UNMATCHED)
    assert np.array_equal(np.delete(got, [before, before + 1], axis=1), expected)
    # offsets that disagree: the pair count of group 3 (5 x 2) is one short
    flat, po, go, eo = pack(tables)
    eo = eo.copy()
    eo[4:] -= 1
    got, pad, status = run_match(flat[:-1], po, go, eo, criteria[:5])
    c0 = int(po[3])
    assert status == 1 and np.all(pad == FILL) and np.all(got[:, c0:c0 + 5] == twin.UNMATCHED)
    assert np.array_equal(got[:, :c0], expected[:5, :c0])


def test_match_twice_gives_the_same_bytes(match_case):
    B, tables, criteria, expected = match_case
    a, _, _ = run_match(*pack(tables), criteria)
    b, _, _ = run_match(*pack(tables), criteria)
    assert a.tobytes() == b.tobytes()


# ---- sdfr_ap_integrate ----------------------------------------------------------------------------------------------
CLASS_SIZES = [0, 1, 63, 64, 65, 1000, 5]     # the last class has no ground truth


def run_integrate(matched, order, class_offset, n_gt):
    lib = _lib()
    T, P = matched.shape
    C = len(n_gt)
    m, o = dev(matched, torch.uint8), dev(order, torch.int32)
    co, ng = dev(class_offset, torch.int32), dev(n_gt, torch.int32)
    ap = torch.full((T, C), -7.0, dtype=torch.float64, device=DEV)
    lib.check(lib.lib().sdfr_ap_integrate(m.data_ptr(), T, P, o.data_ptr(), co.data_ptr(), ng.data_ptr(), C,
                                          ap.data_ptr(), 0, torch.cuda.current_stream().cuda_stream), "sdfr_ap_integrate")
    return ap.cpu().numpy()


@pytest.fixture(scope="module")
def integrate_case():
    rng = np.random.default_rng(4)
    P = sum(CLASS_SIZES)
    order = rng.permutation(P)
    class_offset = np.concatenate([[0], np.cumsum(CLASS_SIZES)])
    n_gt = np.array([3, 1, 63, 64, 65, 1000, 0])
    matched = np.stack([np.where(rng.random(P) < 0.6, rng.integers(0, 64, P), twin.UNMATCHED),
                        np.where(rng.random(P) < 0.1, rng.integers(0, 64, P), twin.UNMATCHED),
                        rng.integers(0, 64, P), np.full(P, twin.UNMATCHED)]).astype(np.uint8)
    return matched, order, class_offset, n_gt, twin.integrate(matched, order, class_offset, n_gt)


def test_integrate_equals_the_twin(integrate_case):
    matched, order, class_offset, n_gt, expected = integrate_case
    got = run_integrate(matched, order, class_offset, n_gt)
    assert got.shape == expected.shape == (4, 7)
    assert np.array_equal(np.isnan(got), np.isnan(expected)) and np.all(np.isnan(got[:, 6]))
    ok = ~np.isnan(expected)
    print("worst |ap - twin| =", np.max(np.abs(got[ok] - expected[ok])))
    assert np.all(np.abs(got[ok] - expected[ok]) <= 1e-12)
    assert np.all(got[:, 0] == 0.0)                                   # ground truths but no detections
    assert np.all(got[2, 1:6] == 1.0) and np.all(got[3, :6] == 0.0)   # all matched, none matched: exactly
    assert 0.0 < got[0, 5] < 1.0
    again = run_integrate(matched, order, class_offset, n_gt)
    assert got.tobytes() == again.tobytes()


# ---- sdfr_pose_pair_errors ------------------------------------------------------------------------------------------
def run_errors(pose_a, pose_b, axis=None):
    from sdfest_amd import ap
    d, s = ap.pose_pair_errors(dev(pose_a, torch.float64), dev(pose_b, torch.float64),
                               None if axis is None else dev(axis, torch.int32))
    return d.cpu().numpy(), s.cpu().numpy()


def test_pose_pair_errors_closed_forms():
    p, I = [0.1, 0.2, 0.3], [0.0, 0.0, 0.0, 1.0]
    q = [0.3, -0.5, 0.2, 0.7]
    half_x = [1.0, 0.0, 0.0, 0.0]
    neg = [-v for v in q]
    a = np.array([p + q, p + q, p + I, p + q, p + I, p + I, [np.nan, 0.0, 0.0] + I])
    b = np.array([p + q, p + neg, p + half_x, p + q, p + half_x, p + [0.0] * 4, p + I])
    axis = np.array([-1, -1, -1, 1, 2, -1, -1])
    degrees, distance = run_errors(a, b, axis)
    assert degrees[0] == 0.0 and distance[0] == 0.0                   # equal poses: exactly
    assert degrees[1] == 0.0 and distance[1] == 0.0                   # q against -q
    assert abs(degrees[2] - 180.0) <= 1e-12                           # a half turn
    assert degrees[3] == 0.0                                          # a symmetry axis with parallel images
    assert abs(degrees[4] - 180.0) <= 1e-12                           # ... with anti-parallel images
    assert np.isnan(degrees[5]) and np.isnan(distance[5])             # a zero quaternion
    assert np.isnan(degrees[6]) and np.isnan(distance[6])             # a non-finite pose
    # without the symmetry array: every pair as axis -1
    d2, s2 = run_errors(a[:3], b[:3])
    assert d2.tobytes() == degrees[:3].tobytes() and s2.tobytes() == distance[:3].tobytes()


def test_pose_pair_errors_equal_the_twin():
    rng = np.random.default_rng(6)
    N = 300                                                           # more than one workgroup
    a = np.concatenate([rng.normal(size=(N, 3)), rng.normal(size=(N, 4))], 1)
    b = np.concatenate([a[:, :3] + rng.normal(size=(N, 3)) * 0.1, rng.normal(size=(N, 4))], 1)
    b[:40, 3:] = a[:40, 3:] + rng.normal(size=(40, 4)) * 1e-9        # nearly equal orientations: where acos would fail
    b[40:80, 3:] = -a[40:80, 3:] * 2.5 + rng.normal(size=(40, 4)) * 1e-7
    axis = rng.integers(-1, 3, N)
    degrees, distance = run_errors(a, b, axis)
    ref_d, ref_s = twin.pose_pair_errors(a, b, [None if k < 0 else k for k in axis])
    print("worst degrees error", np.max(np.abs(degrees - ref_d)), "worst distance error in ulp",
          np.max(np.abs(distance - ref_s) / np.spacing(ref_s)))
    assert np.all(np.abs(degrees - ref_d) <= 1e-12)
    assert np.all(np.abs(distance - ref_s) <= 4 * np.spacing(ref_s))
    again = run_errors(a, b, axis)
    assert again[0].tobytes() == degrees.tobytes() and again[1].tobytes() == distance.tobytes()


# ---- mean_average_precision end to end ------------------------------------------------------------------------------
IOU_T = [0.25, 0.5, 0.75]
DEG_T = [5.0, 10.0, 20.0]
DIST_T = [0.02, 0.05, 0.1]
SYMMETRIC_CLASS, SYMMETRY_AXIS = 5, 1


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def make_scene(seed=21):
    """3 frames, classes 2 and 5 (5 is symmetric about its y axis), 1 .. 5 objects per group; detections are the ground
    truths moved by seeded offsets (a symmetric object also spun about its axis), one is missing, one is spurious"""
    rng = np.random.default_rng(seed)
    counts = {(0, 2): 5, (0, 5): 2, (1, 2): 1, (1, 5): 4, (2, 2): 3, (2, 5): 2}
    gt = {k: [] for k in ("frame", "class_id", "position", "orientation", "extents", "symmetry_axis")}
    det = {k: [] for k in ("frame", "class_id", "position", "orientation", "extents", "score")}
    for (f, c), n in counts.items():
        for k in range(n):
            q = rng.normal(size=4)
            q /= np.linalg.norm(q)
            p = np.array([0.3 * k, 0.1 * c, -1.0]) + rng.normal(size=3) * 0.03
            e = rng.uniform(0.1, 0.25, 3)
            for d, vals in ((gt, (f, c, p, q, e)),):
                for name, v in zip(("frame", "class_id", "position", "orientation", "extents"), vals):
                    d[name].append(v)
            gt["symmetry_axis"].append(SYMMETRY_AXIS if c == SYMMETRIC_CLASS else -1)
            if (f, c, k) == (1, 5, 2):
                continue                                             # the missed object
            turn = rng.normal(size=3)
            turn *= np.deg2rad(rng.uniform(1.0, 25.0)) / 2 / np.linalg.norm(turn)
            dq = qmul(q, np.append(np.sin(np.linalg.norm(turn)) * turn / np.linalg.norm(turn), np.cos(np.linalg.norm(turn))))
            if c == SYMMETRIC_CLASS:
                spin = rng.uniform(0, np.pi)
                dq = qmul(dq, [0.0, np.sin(spin), 0.0, np.cos(spin)])
            det["frame"].append(f), det["class_id"].append(c)
            det["position"].append(p + rng.normal(size=3) * rng.choice([0.01, 0.04]))
            det["orientation"].append(dq), det["extents"].append(e * rng.uniform(0.85, 1.15, 3))
    det["frame"].append(2), det["class_id"].append(2)                # the spurious detection
    det["position"].append(np.array([0.15, 0.25, -1.05])), det["orientation"].append(np.array([0.1, 0.2, 0.3, 0.9]))
    det["extents"].append(np.array([0.2, 0.2, 0.2]))
    det["score"] = rng.permutation(len(det["frame"])) / 100.0 + 0.1   # distinct
    return {k: np.array(v) for k, v in det.items()}, {k: np.array(v) for k, v in gt.items()}


def twin_iou(det, gt):
    def f(i, j):
        axis = int(gt["symmetry_axis"][j])
        return box_iou_twin.box_intersection((gt["position"][j], gt["orientation"][j], gt["extents"][j]),
                                             (det["position"][i], det["orientation"][i], det["extents"][i]),
                                             None if axis < 0 else axis, 20)[1]
    return f


POSE_GATE = 0.6   # iou_min_for_pose of the gated run


@pytest.fixture(scope="module")
def scene():
    from sdfest_amd import mean_average_precision
    det, gt = make_scene()
    cache = {}

    def pair_iou(i, j):   # the twin's box intersection, once per pair
        if (i, j) not in cache:
            cache[(i, j)] = twin_iou(det, gt)(i, j)
        return cache[(i, j)]

    expected = twin.mean_average_precision(det, gt, IOU_T, DEG_T, DIST_T, pair_iou=pair_iou)
    got = mean_average_precision(det, gt, IOU_T, DEG_T, DIST_T, return_matches=True)
    return det, gt, expected, got, pair_iou


def test_map_scene_is_in_general_position(scene):
    """no pair quantity within 1e-9 of a threshold: the twin's flags and the kernels' are then the same question"""
    expected = scene[2]
    quantities = expected["quantities"]
    assert len(quantities) == 25 + 4 + 1 + 12 + 12 + 4
    for column, thresholds in enumerate((IOU_T + [POSE_GATE], DEG_T, DIST_T)):
        gap = np.min(np.abs(quantities[:, column][:, None] - np.array(thresholds)[None]))
        print("column", column, "closest to a threshold:", gap)
        assert gap > 1e-9


def test_map_matches_and_aps_equal_the_twin(scene):
    det, gt, expected, got, _ = scene
    assert got["classes"].tolist() == [2, 5] and got["n_gt"].tolist() == [9, 8] and got["n_detections"].tolist() == [10, 7]
    assert np.array_equal(got["iou_matched"], expected["iou_matched"])
    assert np.array_equal(got["pose_matched"], expected["pose_matched"])
    assert got["iou_ap"].shape == (2, 3) and got["pose_ap"].shape == (2, 3, 3)
    assert got["iou_map"].shape == (3,) and got["pose_map"].shape == (3, 3)
    for name in ("iou_ap", "pose_ap", "iou_map", "pose_map"):
        print(name, got[name].tolist())
        assert np.all(np.abs(got[name] - expected[name]) <= 1e-12), name
    # the scene decides something: the criteria tell detections apart
    assert expected["pose_ap"].min() < expected["pose_ap"].max() and expected["iou_ap"].min() < expected["iou_ap"].max()
    assert 0.0 < expected["pose_ap"].max() and np.any(expected["iou_matched"] == -1) and np.any(expected["iou_matched"] >= 0)


def test_map_with_an_overlap_gate_and_a_given_iou(scene):
    from sdfest_amd import mean_average_precision
    det, gt, expected, _, pair_iou = scene
    gated = twin.mean_average_precision(det, gt, IOU_T, DEG_T, DIST_T, iou_min_for_pose=POSE_GATE, pair_iou=pair_iou)
    got = mean_average_precision(det, gt, IOU_T, DEG_T, DIST_T, iou_min_for_pose=POSE_GATE, return_matches=True)
    assert np.array_equal(got["pose_matched"], gated["pose_matched"])
    assert np.all(np.abs(got["pose_ap"] - gated["pose_ap"]) <= 1e-12)
    assert np.any(gated["pose_ap"] != expected["pose_ap"])          # the gate decides something
    # the caller's IoU in place of the boxes': a matrix that lets nothing overlap
    given = dict(det, iou=np.zeros((len(det["frame"]), len(gt["frame"]))))
    got = mean_average_precision(given, gt, IOU_T, DEG_T, DIST_T)
    assert np.all(got["iou_ap"] == 0.0) and np.all(np.abs(got["pose_ap"] - expected["pose_ap"]) <= 1e-12)


def test_map_of_the_ground_truths_themselves_is_exactly_one():
    from sdfest_amd import mean_average_precision
    _, gt = make_scene()
    n = len(gt["frame"])
    det = {k: gt[k] for k in ("frame", "class_id", "position", "orientation", "extents")}
    det["score"] = np.random.default_rng(8).permutation(n) / n
    got = mean_average_precision(det, gt, [0.1, 0.5, 0.99], [0.5, 5.0], [0.001, 0.1], iou_min_for_pose=0.99)
    assert np.all(got["iou_ap"] == 1.0) and np.all(got["pose_ap"] == 1.0)
    assert np.all(got["iou_map"] == 1.0) and np.all(got["pose_map"] == 1.0)


def test_map_does_not_depend_on_the_order_of_the_frames(scene):
    from sdfest_amd import mean_average_precision
    det, gt, _, got, _ = scene
    by_frames = lambda d, frames: np.concatenate([np.nonzero(d["frame"] == f)[0] for f in frames])
    det2 = {k: v[by_frames(det, (2, 0, 1))] for k, v in det.items()}
    gt2 = {k: v[by_frames(gt, (2, 0, 1))] for k, v in gt.items()}
    again = mean_average_precision(det2, gt2, IOU_T, DEG_T, DIST_T)
    for name in ("iou_ap", "pose_ap", "iou_map", "pose_map"):
        assert again[name].tobytes() == got[name].tobytes(), name


def test_map_refuses_more_than_64_ground_truths_in_a_group():
    from sdfest_amd import mean_average_precision
    n = 65
    q = np.tile([0.0, 0.0, 0.0, 1.0], (n, 1))
    gt = {"frame": np.zeros(n, int), "class_id": np.ones(n, int), "position": np.zeros((n, 3)), "orientation": q,
          "extents": np.ones((n, 3))}
    det = {k: v[:1] for k, v in gt.items()}
    det["score"] = np.array([0.5])
    with pytest.raises(ValueError, match="64"):
        mean_average_precision(det, gt, [0.5], [5.0], [0.05])


# ---- the command line -----------------------------------------------------------------------------------------------
def test_evaluate_detections_tool_writes_the_api_result(tmp_path):
    from sdfest_amd import mean_average_precision
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import evaluate_detections as tool
    finally:
        sys.path.pop(0)
    det, gt = make_scene()
    folder = tmp_path / "results"
    folder.mkdir()

    def similarity(position, quaternion, scale):
        rt = np.eye(4)
        rt[:3, :3] = twin.rotation(np.asarray(quaternion) / np.linalg.norm(quaternion)) * scale
        rt[:3, 3] = position
        return rt

    for f in range(3):
        di, gj = np.nonzero(det["frame"] == f)[0], np.nonzero(gt["frame"] == f)[0]
        scale = 0.5 + 0.1 * f
        record = {"gt_class_ids": gt["class_id"][gj], "gt_scales": gt["extents"][gj] / scale,
                  "gt_RTs": np.array([similarity(gt["position"][j], gt["orientation"][j], scale) for j in gj]),
                  "gt_handle_visibility": np.array([0 if k % 2 else 1 for k in range(len(gj))]),
                  "pred_class_ids": det["class_id"][di], "pred_scores": det["score"][di],
                  "pred_scales": det["extents"][di] / scale,
                  "pred_RTs": np.array([similarity(det["position"][i], det["orientation"][i], scale) for i in di])}
        with open(folder / f"results_{f:04d}.pkl", "wb") as fh:
            pickle.dump(record, fh)
    options = dict(symmetric_classes=[SYMMETRIC_CLASS], symmetry_axis=SYMMETRY_AXIS, handle_class=2)
    det2, gt2, frames = tool.load_results(str(folder), **options)
    assert frames == 3
    # what the tool reads is what was written: poses and extents to rounding, class 2 symmetric where no handle shows
    assert np.allclose(det2["position"], det["position"], atol=1e-12) and np.allclose(gt2["extents"], gt["extents"], atol=1e-12)
    same = np.abs(np.sum(gt2["orientation"] * gt["orientation"], 1))
    assert np.all(np.abs(same - 1.0) <= 1e-12)
    assert set(gt2["symmetry_axis"][gt2["class_id"] == SYMMETRIC_CLASS]) == {SYMMETRY_AXIS}
    assert set(gt2["symmetry_axis"][gt2["class_id"] == 2]) == {-1, SYMMETRY_AXIS}
    expected = mean_average_precision(det2, gt2, [0.25, 0.5], [5.0, 10.0], [0.02, 0.05, 0.1])
    out = tmp_path / "map.json"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "evaluate_detections.py"), str(folder), "--out", str(out),
           "--symmetric-classes", str(SYMMETRIC_CLASS), "--symmetry-axis", str(SYMMETRY_AXIS), "--handle-class", "2",
           "--iou-thresholds", "0.25", "0.5", "--degree-thresholds", "5", "10", "--distance-thresholds", "0.02", "0.05",
           "0.1"]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "mAP" in done.stdout
    written = json.loads(out.read_text())
    for name, value in expected.items():
        assert np.array_equal(np.array(written[name], dtype=value.dtype), value, equal_nan=value.dtype.kind == "f"), name
    assert written["frames"] == 3
