"""numpy float64 twin of the detection matching and average precision of sdfest_amd/ap.py (csrc/ap.hip): the one
statement of the protocol in plain loops, written for reading.  Imports nothing from the product.

THE PROTOCOL (the project's own, after the published NOCS evaluation; no parity with a third-party script is claimed).
A group is one (frame, class); only its detections and ground truths can match.  Inside a group the detections are
processed by descending score, ties by the lower input index.  Every (detection i, ground truth j) pair of a group has
four numbers: iou, degrees, distance (metres) and key.  A criterion is (iou_min, degrees_max, distance_max); a pair is
admissible iff iou >= iou_min and degrees <= degrees_max and distance <= distance_max, and a pair with a NaN entry never
is.  Criteria are matched independently: in detection order a detection takes the admissible, still unmatched ground
truth with the smallest key (ties: the lower ground-truth index) or stays unmatched.  The AP of one (class, criterion):
all detections of the class over all frames by descending score (ties: the lower input index), tp_k = detection k is
matched, precision_k = cumtp_k / (k + 1), envelope_k = max_{j >= k} precision_j, AP = (sum over the matched k of
envelope_k) / n_gt -- NaN for n_gt == 0, 0 for ground truths without detections.  mAP: the mean over the classes whose
AP is not NaN."""
import numpy as np

UNMATCHED = 255
MAX_GT = 64


# ---- pair errors ----------------------------------------------------------------------------------------------------
def rotation(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pose_pair_error(pose_a, pose_b, symmetry_axis=None):
    """(degrees, distance) of two poses (position (3), quaternion x y z w (4)); symmetry_axis 0 | 1 | 2: the angle between
    the two images of that object axis.  A non-finite entry or a zero quaternion: (nan, nan)."""
    a, b = np.asarray(pose_a, np.float64), np.asarray(pose_b, np.float64)
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
        return np.nan, np.nan
    na, nb = float(a[3:] @ a[3:]), float(b[3:] @ b[3:])
    if not (na > 0 and nb > 0 and np.isfinite(na) and np.isfinite(nb)):
        return np.nan, np.nan
    d = a[:3] - b[:3]
    distance = float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    qa, qb = a[3:] / np.sqrt(na), b[3:] / np.sqrt(nb)
    if symmetry_axis is not None and 0 <= int(symmetry_axis) <= 2:
        u, v = rotation(qa)[:, int(symmetry_axis)], rotation(qb)[:, int(symmetry_axis)]
        c = np.cross(u, v)
        rad = np.arctan2(np.sqrt(c @ c), u @ v)
    else:
        (ax, ay, az, aw), (bx, by, bz, bw) = qa, qb   # qa * conj(qb)
        r = np.array([(ax * bw - aw * bx) + (az * by - ay * bz), (ay * bw - aw * by) + (ax * bz - az * bx),
                      (az * bw - aw * bz) + (ay * bx - ax * by)])
        w = (aw * bw + ax * bx) + (ay * by + az * bz)
        rad = 2.0 * np.arctan2(np.sqrt(r @ r), abs(w))
    return float(rad * (180.0 / np.pi)), distance


def pose_pair_errors(pose_a, pose_b, symmetry_axis=None):
    out = [pose_pair_error(a, b, None if symmetry_axis is None else symmetry_axis[n])
           for n, (a, b) in enumerate(zip(pose_a, pose_b))]
    return np.array([o[0] for o in out], np.float64), np.array([o[1] for o in out], np.float64)


# ---- matching -------------------------------------------------------------------------------------------------------
def match_group(table, criterion):
    """table (nd, ng, 4) of one group, detections in processing order -> per detection the ground-truth index it took,
    or UNMATCHED"""
    iou_min, degrees_max, distance_max = criterion
    nd, ng = table.shape[:2]
    taken = [False] * ng
    out = []
    for i in range(nd):
        best, best_key = UNMATCHED, None
        for j in range(ng):
            iou, degrees, distance, key = table[i, j]
            if taken[j] or np.isnan(key):
                continue
            if not (iou >= iou_min and degrees <= degrees_max and distance <= distance_max):   # false for a NaN
                continue
            if best == UNMATCHED or key < best_key:
                best, best_key = j, key
        if best != UNMATCHED:
            taken[best] = True
        out.append(best)
    return out


def match(table, pred_offset, gt_offset, pair_offset, criteria, P=None):
    """matched (T, P) uint8 of G groups: table (n_pairs, 4), the three offset arrays (G + 1,), criteria (T, 3).  A group
    with more than MAX_GT ground truths or a pair count that is not nd x ng gets UNMATCHED in all its rows; also
    returns whether there was one.  Columns no group covers keep 0."""
    table = np.asarray(table, np.float64).reshape(-1, 4)
    criteria = np.asarray(criteria, np.float64).reshape(-1, 3)
    P = int(pred_offset[-1]) if P is None else P
    matched = np.zeros((len(criteria), P), np.uint8)
    refused = False
    for g in range(len(pred_offset) - 1):
        p0, nd = int(pred_offset[g]), int(pred_offset[g + 1] - pred_offset[g])
        ng = int(gt_offset[g + 1] - gt_offset[g])
        e0, e1 = int(pair_offset[g]), int(pair_offset[g + 1])
        if ng > MAX_GT or e1 - e0 != nd * ng:
            matched[:, p0:p0 + nd] = UNMATCHED
            refused = True
            continue
        t = table[e0:e1].reshape(nd, ng, 4)
        for k, c in enumerate(criteria):
            matched[k, p0:p0 + nd] = match_group(t, c)
    return matched, refused


# ---- average precision ----------------------------------------------------------------------------------------------
def average_precision(tp, n_gt):
    """AP of one (class, criterion): tp = the match flags of the class's detections by descending score"""
    if n_gt == 0:
        return np.nan
    n = len(tp)
    precision, cum = [], 0
    for k in range(n):
        cum += 1 if tp[k] else 0
        precision.append(cum / (k + 1))
    envelope = list(precision)
    for k in range(n - 2, -1, -1):
        envelope[k] = max(envelope[k], envelope[k + 1])
    total = 0.0
    for k in range(n):
        if tp[k]:
            total += envelope[k]
    return total / n_gt


def integrate(matched, order, class_offset, n_gt):
    """ap (T, C): matched (T, P), order (P,) the columns class by class by descending score, class_offset (C + 1,)"""
    T, C = matched.shape[0], len(n_gt)
    ap = np.zeros((T, C))
    for t in range(T):
        for c in range(C):
            cols = order[class_offset[c]:class_offset[c + 1]]
            ap[t, c] = average_precision([matched[t, d] != UNMATCHED for d in cols], int(n_gt[c]))
    return ap


def mean_over_classes(ap, axis=0):
    """the mean over the classes (axis) whose AP is not NaN; NaN where every class is"""
    ap = np.asarray(ap, np.float64)
    ok = ~np.isnan(ap)
    count = ok.sum(axis)
    total = np.where(ok, ap, 0.0).sum(axis)
    return np.where(count > 0, total / np.maximum(count, 1), np.nan)


# ---- end to end -----------------------------------------------------------------------------------------------------
def score_order(indices, score):
    """`indices` by descending score, ties by the lower index"""
    return sorted(indices, key=lambda i: (-float(score[i]), i))


def mean_average_precision(detections, ground_truths, iou_thresholds, degree_thresholds, distance_thresholds,
                           iou_min_for_pose=None, pair_iou=None):
    """The whole evaluation in loops.  detections / ground_truths: dicts of arrays (frame, class_id, position,
    orientation, extents; score; symmetry_axis with -1 for none).  pair_iou(i, j) -> the IoU of detection i and ground
    truth j (the caller brings the box intersection: tests/box_iou_twin.py, or recorded values).  Returns the product's
    dict plus "iou_matched" (Ti, Nd) and "pose_matched" (D S, Nd): per detection, in INPUT order, the INPUT index of the
    ground truth it took, or -1."""
    det, gt = detections, ground_truths
    nd, ng = len(det["frame"]), len(gt["frame"])
    classes = sorted(set(int(c) for c in det["class_id"]) | set(int(c) for c in gt["class_id"]))
    groups = sorted(set((int(f), int(c)) for f, c in zip(det["frame"], det["class_id"])) |
                    set((int(f), int(c)) for f, c in zip(gt["frame"], gt["class_id"])))
    iou_criteria = [(t, np.inf, np.inf) for t in iou_thresholds]
    lo = -np.inf if iou_min_for_pose is None else iou_min_for_pose
    pose_criteria = [(lo, d, s) for d in degree_thresholds for s in distance_thresholds]
    iou_matched = -np.ones((len(iou_criteria), nd), np.int64)
    pose_matched = -np.ones((len(pose_criteria), nd), np.int64)
    quantities = []   # every pair's (iou, degrees, distance): what the thresholds are compared with
    for f, c in groups:
        di = score_order([i for i in range(nd) if (int(det["frame"][i]), int(det["class_id"][i])) == (f, c)], det["score"])
        gj = [j for j in range(ng) if (int(gt["frame"][j]), int(gt["class_id"][j])) == (f, c)]
        if len(gj) > MAX_GT:
            raise ValueError(f"frame {f}, class {c}: {len(gj)} ground truths")
        table = np.zeros((len(di), len(gj), 4))
        for a, i in enumerate(di):
            for b, j in enumerate(gj):
                axis = int(gt["symmetry_axis"][j])
                degrees, distance = pose_pair_error(np.concatenate([gt["position"][j], gt["orientation"][j]]),
                                                    np.concatenate([det["position"][i], det["orientation"][i]]),
                                                    axis if axis >= 0 else None)
                table[a, b, :3] = pair_iou(i, j), degrees, distance
                quantities.append(table[a, b, :3].copy())
        for out, criteria, key in ((iou_matched, iou_criteria, -table[..., 0]),
                                   (pose_matched, pose_criteria, table[..., 1] + 100.0 * table[..., 2])):
            table[..., 3] = key
            for t, crit in enumerate(criteria):
                for a, m in enumerate(match_group(table, crit)):
                    out[t, di[a]] = gj[m] if m != UNMATCHED else -1
    C = len(classes)
    n_gt = [sum(1 for j in range(ng) if int(gt["class_id"][j]) == c) for c in classes]
    n_det = [sum(1 for i in range(nd) if int(det["class_id"][i]) == c) for c in classes]
    by_class = [score_order([i for i in range(nd) if int(det["class_id"][i]) == c], det["score"]) for c in classes]
    ap_of = lambda m: np.array([[average_precision([m[t, i] >= 0 for i in by_class[k]], n_gt[k])
                                 for t in range(m.shape[0])] for k in range(C)]).reshape(C, m.shape[0])
    iou_ap = ap_of(iou_matched)
    pose_ap = ap_of(pose_matched).reshape(C, len(degree_thresholds), len(distance_thresholds))
    return {"classes": np.array(classes, np.int64), "iou_ap": iou_ap, "pose_ap": pose_ap,
            "iou_map": mean_over_classes(iou_ap), "pose_map": mean_over_classes(pose_ap),
            "n_gt": np.array(n_gt, np.int64), "n_detections": np.array(n_det, np.int64),
            "iou_matched": iou_matched, "pose_matched": pose_matched,
            "quantities": np.array(quantities).reshape(-1, 3)}
