"""CPU: the numpy twin of the detection matching and average precision (tests/ap_twin.py) on hand-worked cases, the
host bookkeeping of sdfest_amd/ap.py on the CPU device against the twin's loops, and the argument errors of the three
entry points of include/sdfr.h group 16, which are reported before any HIP call."""
import ctypes
import math

import numpy as np
import pytest

import ap_twin as twin

INF = float("inf")


def table_of(rows):
    """(nd, ng, 4) from nested [[(iou, degrees, distance, key), ...], ...]"""
    return np.array(rows, np.float64)


# ---- the AP integral ------------------------------------------------------------------------------------------------
def test_tp_fp_tp_against_two_ground_truths():
    tp = [True, False, True]
    precision = [1.0, 1.0 / 2.0, 2.0 / 3.0]
    envelope = [1.0, 2.0 / 3.0, 2.0 / 3.0]
    assert [max(precision[k:]) for k in range(3)] == envelope
    assert twin.average_precision(tp, 2) == (1.0 + 2.0 / 3.0) / 2.0
    # through the column bookkeeping: one class, the columns given out of order
    matched = np.array([[twin.UNMATCHED, 0, 1]], np.uint8)          # column 0 is the false positive
    ap = twin.integrate(matched, order=[1, 0, 2], class_offset=[0, 3], n_gt=[2])
    assert ap.shape == (1, 1) and ap[0, 0] == (1.0 + 2.0 / 3.0) / 2.0


@pytest.mark.parametrize("n", [1, 3, 64, 1000])
def test_all_matched_is_exactly_one_and_none_matched_exactly_zero(n):
    assert twin.average_precision([True] * n, n) == 1.0
    assert twin.average_precision([False] * n, n) == 0.0
    assert twin.average_precision([], 4) == 0.0                       # ground truths but no detections


def test_class_without_ground_truths_is_nan_and_left_out_of_the_mean():
    assert math.isnan(twin.average_precision([False, False], 0))
    assert math.isnan(twin.average_precision([], 0))
    ap = np.array([[0.5, np.nan, 1.0], [np.nan, np.nan, np.nan]]).T     # (C = 3, T = 2)
    mean = twin.mean_over_classes(ap)
    assert mean[0] == 0.75 and math.isnan(mean[1])


# ---- matching -------------------------------------------------------------------------------------------------------
def test_smallest_key_wins_and_a_taken_ground_truth_is_gone():
    t = table_of([[(0.6, 0, 0, -0.6), (0.9, 0, 0, -0.9)],
                  [(0.5, 0, 0, -0.5), (0.8, 0, 0, -0.8)]])
    assert twin.match_group(t, (0.25, INF, INF)) == [1, 0]
    assert twin.match_group(t, (0.7, INF, INF)) == [1, twin.UNMATCHED]   # 0.5 is not admissible, 1 is taken
    assert twin.match_group(t, (0.95, INF, INF)) == [twin.UNMATCHED] * 2


def test_tie_in_key_goes_to_the_lower_ground_truth_index():
    t = table_of([[(0.5, 1, 1, 7.0), (0.5, 1, 1, 7.0), (0.5, 1, 1, 7.0)]] * 2)
    assert twin.match_group(t, (-INF, INF, INF)) == [0, 1]


def test_value_exactly_at_a_threshold_is_admissible():
    t = table_of([[(0.25, 10.0, 0.05, 0.0)]])
    assert twin.match_group(t, (0.25, 10.0, 0.05)) == [0]
    assert twin.match_group(t, (np.nextafter(0.25, 1), 10.0, 0.05)) == [twin.UNMATCHED]
    assert twin.match_group(t, (0.25, np.nextafter(10.0, 0), 0.05)) == [twin.UNMATCHED]
    assert twin.match_group(t, (0.25, 10.0, np.nextafter(0.05, 0))) == [twin.UNMATCHED]


def test_nan_entries_are_never_admissible():
    for column in range(4):
        row = [0.5, 1.0, 0.01, 0.0]
        row[column] = np.nan
        assert twin.match_group(table_of([[tuple(row)]]), (-INF, INF, INF)) == [twin.UNMATCHED]


def test_refused_groups_in_the_twin():
    table = np.zeros((65, 4))
    matched, refused = twin.match(table, [0, 1], [0, 65], [0, 65], [(-INF, INF, INF)])
    assert refused and matched.tolist() == [[twin.UNMATCHED]]


def _two_frame_set():
    """frame 0: two detections with EQUAL scores over one ground truth; frame 1: one detection, one ground truth"""
    q = [0.0, 0.0, 0.0, 1.0]
    det = {"frame": np.array([0, 0, 1]), "class_id": np.array([3, 3, 3]), "score": np.array([0.5, 0.5, 0.9]),
           "position": np.array([[0.0, 0, 0], [0.0, 0, 0], [1.0, 0, 0]]), "orientation": np.array([q] * 3),
           "extents": np.ones((3, 3))}
    gt = {"frame": np.array([0, 1]), "class_id": np.array([3, 3]), "position": np.array([[0.0, 0, 0], [1.0, 0, 0]]),
          "orientation": np.array([q] * 2), "extents": np.ones((2, 3)), "symmetry_axis": np.array([-1, -1])}
    return det, gt


def test_tie_in_score_goes_to_the_lower_input_index():
    det, gt = _two_frame_set()
    out = twin.mean_average_precision(det, gt, [0.5], [5.0], [0.01], pair_iou=lambda i, j: 1.0)
    # detection 0 and 1 tie: 0 is processed first and takes the ground truth
    assert out["iou_matched"].tolist() == [[0, -1, 1]] and out["pose_matched"].tolist() == [[0, -1, 1]]
    # by descending score the class's flags are 2 (tp), 0 (tp), 1 (fp): both ground truths found before the miss
    assert out["iou_ap"].tolist() == [[1.0]] and out["n_gt"].tolist() == [2] and out["n_detections"].tolist() == [3]
    assert twin.score_order([0, 1, 2], det["score"]) == [2, 0, 1]


def test_pose_pair_error_closed_forms():
    p, I = [0.1, 0.2, 0.3], [0.0, 0.0, 0.0, 1.0]
    q = np.array([0.3, -0.5, 0.2, 0.7])
    assert twin.pose_pair_error(p + list(q), p + list(q)) == (0.0, 0.0)
    assert twin.pose_pair_error(p + list(q), p + list(-q)) == (0.0, 0.0)
    assert twin.pose_pair_error(p + list(q), p + list(3.0 * q))[0] <= 1e-13          # normalised inside
    assert abs(twin.pose_pair_error(p + I, p + [1.0, 0.0, 0.0, 0.0])[0] - 180.0) <= 1e-12
    assert twin.pose_pair_error(p + I, [0.1, 0.2, 0.8] + I) == (0.0, 0.5)
    # a turn about the symmetry axis is not seen; a half turn about another axis turns the axis round
    turn_z = [0.0, 0.0, math.sin(0.4), math.cos(0.4)]
    assert twin.pose_pair_error(p + I, p + turn_z, 2)[0] == 0.0
    assert abs(twin.pose_pair_error(p + I, p + turn_z)[0] - math.degrees(0.8)) <= 1e-12
    assert abs(twin.pose_pair_error(p + I, p + [1.0, 0.0, 0.0, 0.0], 2)[0] - 180.0) <= 1e-12
    assert all(math.isnan(v) for v in twin.pose_pair_error(p + I, p + [0.0] * 4))
    assert all(math.isnan(v) for v in twin.pose_pair_error([np.inf, 0, 0] + I, p + I))


# ---- the host bookkeeping, on the CPU device ------------------------------------------------------------------------
def test_group_detections_bookkeeping_matches_the_loops():
    import torch
    from sdfest_amd import ap
    rng = np.random.default_rng(5)
    nd, ng = 40, 37
    det_frame, det_class = rng.integers(0, 4, nd), rng.choice([2, 5, 9], nd)
    gt_frame, gt_class = rng.integers(0, 5, ng), rng.choice([2, 5, 7], ng)
    score = rng.integers(0, 6, nd) / 4.0                                  # many ties
    g = ap.group_detections(det_frame, det_class, score, gt_frame, gt_class, device=torch.device("cpu"))
    classes = sorted(set(det_class) | set(gt_class))
    groups = sorted(set(zip(det_frame, det_class)) | set(zip(gt_frame, gt_class)))
    assert g.classes.tolist() == classes and (g.G, g.P, g.C) == (len(groups), nd, len(classes))
    det_order, gt_order, pair_det, pair_gt = [], [], [], []
    for f, c in groups:
        di = twin.score_order([i for i in range(nd) if (det_frame[i], det_class[i]) == (f, c)], score)
        gj = [j for j in range(ng) if (gt_frame[j], gt_class[j]) == (f, c)]
        k = groups.index((f, c))
        assert (g.pred_offset[k].item(), g.gt_offset[k].item(), g.pair_offset[k].item()) == (len(det_order), len(gt_order),
                                                                                           len(pair_det))
        det_order += di
        gt_order += gj
        pair_det += [i for i in di for _ in gj]
        pair_gt += [j for _ in di for j in gj]
    assert g.det_order.tolist() == det_order and g.gt_order.tolist() == gt_order
    assert g.pair_det.tolist() == pair_det and g.pair_gt.tolist() == pair_gt and g.n_pairs == len(pair_det)
    assert g.pred_offset[-1].item() == nd and g.gt_offset[-1].item() == ng and g.pair_offset[-1].item() == len(pair_det)
    assert g.max_gt == max(sum(1 for j in range(ng) if (gt_frame[j], gt_class[j]) == k) for k in groups)
    by_class = [i for c in classes for i in twin.score_order([i for i in range(nd) if det_class[i] == c], score)]
    assert [det_order[p] for p in g.order.tolist()] == by_class
    assert g.n_gt.tolist() == [int((gt_class == c).sum()) for c in classes]
    assert g.n_detections.tolist() == [int((det_class == c).sum()) for c in classes]
    assert g.class_offset.tolist() == [0] + list(np.cumsum(g.n_detections.tolist()))
    with pytest.raises(ValueError, match="finite"):
        ap.group_detections([0], [1], [np.nan], [0], [1], device=torch.device("cpu"))


def test_exports():
    import sdfest_amd
    from sdfest_amd import ap, metrics
    assert sdfest_amd.mean_average_precision is ap.mean_average_precision is metrics.mean_average_precision
    assert "mean_average_precision" in sdfest_amd.__all__ and "mean_average_precision" in metrics.__all__
    assert (ap.MAX_GT, ap.UNMATCHED) == (twin.MAX_GT, twin.UNMATCHED) == (64, 255)


# ---- the C ABI's argument errors ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from sdfest_amd import _lib
    _lib.build()
    return _lib.lib()


def test_entry_points_validate_their_arguments_without_gpu(L):
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)            # a non-NULL, 8-byte aligned pointer that is never dereferenced
    odd = ctypes.c_void_p(q.value + 4)               # 4-byte aligned only
    odd2 = ctypes.c_void_p(q.value + 2)
    err = lambda: L.sdfr_last_error()
    # sdfr_pose_pair_errors(pose_a, pose_b, symmetry_axis, N, degrees, distance, device, stream)
    assert L.sdfr_pose_pair_errors(q, q, None, -1, q, q, 0, None) == -1 and b"N=-1" in err()
    assert L.sdfr_pose_pair_errors(None, None, None, 0, None, None, 0, None) == 0               # nothing to do
    assert L.sdfr_pose_pair_errors(None, q, None, 1, q, q, 0, None) == -2 and b"NULL" in err()
    assert L.sdfr_pose_pair_errors(q, q, None, 1, q, None, 0, None) == -2
    assert L.sdfr_pose_pair_errors(q, odd, None, 1, q, q, 0, None) == -1 and b"8-byte aligned" in err()
    assert L.sdfr_pose_pair_errors(q, q, odd2, 1, q, q, 0, None) == -1 and b"4-byte aligned" in err()
    # sdfr_ap_match(table, n_pairs, pred_offset, gt_offset, pair_offset, G, P, criteria, T, matched, status, device, stream)
    assert L.sdfr_ap_match(q, -1, q, q, q, 1, 1, q, 1, q, None, 0, None) == -1 and b"n_pairs=-1" in err()
    assert L.sdfr_ap_match(q, 1, q, q, q, -1, 1, q, 1, q, None, 0, None) == -1
    assert L.sdfr_ap_match(q, 1, q, q, q, 1, -1, q, 1, q, None, 0, None) == -1
    assert L.sdfr_ap_match(q, 1, q, q, q, 1, 1, q, -1, q, None, 0, None) == -1
    assert L.sdfr_ap_match(q, 1, q, q, q, (1 << 24) + 1, 1, q, 1, q, None, 0, None) == -1 and b"G=" in err()
    assert L.sdfr_ap_match(q, 1, q, q, q, 1, 1, q, (1 << 20) + 1, q, None, 0, None) == -1 and b"T=" in err()
    for G, P, T in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):                                            # nothing to do
        assert L.sdfr_ap_match(None, 0, None, None, None, G, P, None, T, None, None, 0, None) == 0
    assert L.sdfr_ap_match(None, 1, q, q, q, 1, 1, q, 1, q, None, 0, None) == -2 and b"NULL" in err()
    for k in (2, 3, 4, 7, 9):
        args = [q, 1, q, q, q, 1, 1, q, 1, q, None, 0, None]
        args[k] = None
        assert L.sdfr_ap_match(*args) == -2, k
    assert L.sdfr_ap_match(odd, 1, q, q, q, 1, 1, q, 1, q, None, 0, None) == -1 and b"8-byte aligned" in err()
    assert L.sdfr_ap_match(q, 1, q, q, odd, 1, 1, q, 1, q, None, 0, None) == -1
    assert L.sdfr_ap_match(q, 1, q, q, q, 1, 1, odd, 1, q, None, 0, None) == -1
    assert L.sdfr_ap_match(q, 1, odd2, q, q, 1, 1, q, 1, q, None, 0, None) == -1 and b"4-byte aligned" in err()
    assert L.sdfr_ap_match(q, 1, q, q, q, 1, 1, q, 1, q, odd2, 0, None) == -1
    # sdfr_ap_integrate(matched, T, P, order, class_offset, n_gt, C, ap, device, stream)
    assert L.sdfr_ap_integrate(q, -1, 1, q, q, q, 1, q, 0, None) == -1 and b"T=-1" in err()
    assert L.sdfr_ap_integrate(q, 1, -1, q, q, q, 1, q, 0, None) == -1
    assert L.sdfr_ap_integrate(q, 1, 1, q, q, q, -1, q, 0, None) == -1
    assert L.sdfr_ap_integrate(q, (1 << 20) + 1, 1, q, q, q, 1, q, 0, None) == -1 and b"T=" in err()
    assert L.sdfr_ap_integrate(q, 1 << 20, 1, q, q, q, 1 << 12, q, 0, None) == -1 and b"int32" in err()
    assert L.sdfr_ap_integrate(None, 0, 1, None, None, None, 1, None, 0, None) == 0
    assert L.sdfr_ap_integrate(None, 1, 1, None, None, None, 0, None, 0, None) == 0
    for k in (0, 3, 4, 5, 7):
        args = [q, 1, 1, q, q, q, 1, q, 0, None]
        args[k] = None
        assert L.sdfr_ap_integrate(*args) == -2 and b"NULL" in err(), k
    assert L.sdfr_ap_integrate(q, 1, 1, q, q, q, 1, odd, 0, None) == -1 and b"8-byte aligned" in err()
    assert L.sdfr_ap_integrate(q, 1, 1, odd2, q, q, 1, q, 0, None) == -1 and b"4-byte aligned" in err()
