"""Detection matching and average precision on the GPU (``sdfr_pose_pair_errors`` / ``sdfr_ap_match`` /
``sdfr_ap_integrate``, csrc/ap.hip): AP over IoU thresholds and over (degrees, distance) thresholds, per class and
averaged -- the number category-level pose estimation reports.  The heavy steps are the three kernels and ``box_iou``;
torch only sorts, gathers and concatenates.

THE PROTOCOL is the project's own statement, after the published NOCS evaluation (include/sdfr.h group 16 and DESIGN.md
section 3.22 state it in full; tests/ap_twin.py restates it in numpy loops); parity with a third-party script is not
claimed.  A group is one (frame, class) and only its detections and ground truths can match; inside a group detections
are processed by descending score (ties: the lower input index); every pair has (iou, degrees, distance, key); a
criterion (iou_min, degrees_max, distance_max) admits a pair iff ``iou >= iou_min and degrees <= degrees_max and
distance <= distance_max`` (a NaN never passes); under each criterion, independently, a detection takes the admissible,
still unmatched ground truth with the smallest key (ties: the lower ground-truth index).  AP = (the sum over the matched
detections, by descending score, of the precision envelope) / n_gt; NaN for a class without ground truths, which the
mean over classes leaves out.

``detections`` and ``ground_truths`` are dicts of arrays or tensors: ``frame`` (N,), ``class_id`` (N,) integers,
``position`` (N,3) metres, ``orientation`` (N,4) quaternions x y z w, ``extents`` (N,3) full side lengths; detections
also ``score`` (N,), ground truths optionally ``symmetry_axis`` (N,) in {-1, 0, 1, 2}; detections optionally ``iou``
(Nd, Ngt), the caller's own IoU of every detection (row) against every ground truth (column) in input order, used in
place of the oriented boxes' (another IoU definition can then be scored; the matrix is dense, so this is for result sets
whose Nd x Ngt doubles fit)."""
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .boxes import box_iou

__all__ = ["DetectionGroups", "group_detections", "pair_table", "with_key", "pose_pair_errors", "match_detections",
           "average_precision", "mean_average_precision"]

MAX_GT = _lib.ABI["SDFR_AP_MAX_GT"]
UNMATCHED = _lib.ABI["SDFR_AP_UNMATCHED"]


def _device(*dicts) -> torch.device:
    for d in dicts:
        for v in d.values():
            if isinstance(v, torch.Tensor) and v.is_cuda:
                return v.device
    return torch.device("cuda", torch.cuda.current_device())


def _field(d: dict, name: str, width: int, dtype, dev, n: Optional[int] = None, default=None) -> torch.Tensor:
    if name not in d or d[name] is None:
        if default is None:
            raise ValueError(f"'{name}' is missing")
        return torch.full((n,), default, dtype=dtype, device=dev)
    v = d[name]
    t = v.detach() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
    shape = (t.shape[0],) if width == 0 else (t.shape[0], width)
    if t.dim() != len(shape) or tuple(t.shape) != shape or (n is not None and t.shape[0] != n):
        raise ValueError(f"'{name}': shape ({'N' if n is None else n}{',' + str(width) if width else ''}) expected, got "
                         f"{tuple(t.shape)}")
    return t.to(device=dev, dtype=dtype).contiguous()


def _offsets(counts: torch.Tensor, dtype) -> torch.Tensor:
    return torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(dtype)


class DetectionGroups:
    """The bookkeeping of one result set, all on the device: which column of ``matched`` is which detection, the groups'
    offsets, the table's rows, and each class's slice.

    classes (C,) int64 sorted class ids; G groups, P detections, n_pairs table rows, max_gt the largest group's ground
    truths.  det_order (P,): the INPUT index of the detection in column p (group by group, each by descending score);
    gt_order (Ngt,): the input index of a ground truth, group by group in input order; column_group (P,): the group of a
    column; pred_offset, gt_offset (G+1,) int32, pair_offset (G+1,) int64; pair_det, pair_gt (n_pairs,): the input
    indices of a table row's detection and ground truth; order (P,) int32: the columns class by class, each by
    descending score (ties: the lower input index); class_offset (C+1,) int32; n_gt, n_detections (C,) int32."""

    def __init__(self, **kw) -> None:
        self.__dict__.update(kw)


def group_detections(det_frame, det_class, det_score, gt_frame, gt_class, device=None) -> DetectionGroups:
    """Sort one result set into groups (sorts and gathers only; one host read for the sizes)."""
    dev = device or torch.device("cuda", torch.cuda.current_device())
    as_long = lambda v: (v.detach() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))).to(dev, torch.int64)
    df, dc, gf, gc = as_long(det_frame), as_long(det_class), as_long(gt_frame), as_long(gt_class)
    score = (det_score.detach() if isinstance(det_score, torch.Tensor) else torch.as_tensor(np.asarray(det_score))).to(
        dev, torch.float64)
    P, Ngt = int(df.shape[0]), int(gf.shape[0])
    if not (dc.shape == df.shape == score.shape and df.dim() == 1 and gc.shape == gf.shape and gf.dim() == 1):
        raise ValueError("frame, class_id (and score) must be one-dimensional and equally long")
    frames, classes = torch.unique(torch.cat([df, gf])), torch.unique(torch.cat([dc, gc]))
    C = int(classes.numel())
    dci, gci = torch.searchsorted(classes, dc), torch.searchsorted(classes, gc)
    dkey, gkey = torch.searchsorted(frames, df) * C + dci, torch.searchsorted(frames, gf) * C + gci
    keys = torch.unique(torch.cat([dkey, gkey]))
    G = int(keys.numel())
    dg, gg = torch.searchsorted(keys, dkey), torch.searchsorted(keys, gkey)
    by_score = torch.sort(-score, stable=True).indices            # descending score, ties: the lower input index
    det_order = by_score[torch.sort(dg[by_score], stable=True).indices]
    gt_order = torch.sort(gg, stable=True).indices
    nd, ng = torch.bincount(dg, minlength=G), torch.bincount(gg, minlength=G)
    pred_offset, gt_offset, pair_offset = _offsets(nd, torch.int64), _offsets(ng, torch.int64), _offsets(nd * ng, torch.int64)
    by_class = by_score[torch.sort(dci[by_score], stable=True).indices]
    column_of = torch.empty(P, dtype=torch.int64, device=dev)
    column_of[det_order] = torch.arange(P, device=dev)
    n_det, n_gt = torch.bincount(dci, minlength=C), torch.bincount(gci, minlength=C)
    sizes = torch.stack([pair_offset[-1], ng.max() if G else pair_offset[0],
                         torch.isfinite(score).all().to(torch.int64)]).cpu().numpy()        # the one host read
    if not sizes[2]:
        raise ValueError("detection scores must be finite")
    n_pairs, max_gt = int(sizes[0]), int(sizes[1])
    e = torch.arange(n_pairs, device=dev)
    pg = torch.searchsorted(pair_offset, e, right=True) - 1
    local = e - pair_offset[pg]
    width = ng[pg].clamp(min=1)
    pair_det = det_order[pred_offset[pg] + local // width]
    pair_gt = gt_order[gt_offset[pg] + local % width]
    return DetectionGroups(
        device=dev, classes=classes, G=G, P=P, C=C, n_pairs=n_pairs, max_gt=max_gt, det_order=det_order,
        gt_order=gt_order, column_group=dg[det_order], pred_offset=pred_offset.to(torch.int32),
        gt_offset=gt_offset.to(torch.int32), pair_offset=pair_offset, pair_det=pair_det, pair_gt=pair_gt,
        order=column_of[by_class].to(torch.int32), class_offset=_offsets(n_det, torch.int32),
        n_gt=n_gt.to(torch.int32), n_detections=n_det.to(torch.int32))


def pose_pair_errors(pose_a: torch.Tensor, pose_b: torch.Tensor, symmetry_axis: Optional[torch.Tensor] = None):
    """(degrees (N,), distance (N,)) float64 of N pose pairs: pose rows (N,7) = position, quaternion x y z w (normalised
    inside), CUDA tensors; symmetry_axis (N,) int in {-1, 0, 1, 2} or None.  degrees = 2 atan2(|v|, |w|) of the relative
    quaternion, or with an axis the angle between the two images of that object axis; distance = |p_a - p_b|; NaN in both
    for a non-finite pose or a zero quaternion.  One launch, nothing read back."""
    if pose_a.dim() != 2 or pose_a.shape[1] != 7 or pose_a.shape != pose_b.shape:
        raise ValueError(f"poses: two (N,7) tensors expected, got {tuple(pose_a.shape)} and {tuple(pose_b.shape)}")
    if not pose_a.is_cuda:
        raise TypeError("poses must be CUDA tensors (sdfest_amd has no CPU path)")
    dev = pose_a.device
    a = pose_a.detach().to(torch.float64).contiguous()
    b = pose_b.detach().to(device=dev, dtype=torch.float64).contiguous()
    N = int(a.shape[0])
    axis = None
    if symmetry_axis is not None:
        axis = symmetry_axis.detach().to(device=dev, dtype=torch.int32).contiguous()
        if tuple(axis.shape) != (N,):
            raise ValueError(f"symmetry_axis: shape ({N},) expected, got {tuple(axis.shape)}")
    degrees = torch.empty(N, dtype=torch.float64, device=dev)
    distance = torch.empty(N, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sdfr_pose_pair_errors(a.data_ptr(), b.data_ptr(), None if axis is None else axis.data_ptr(),
                                                    N, degrees.data_ptr(), distance.data_ptr(), dev.index,
                                                    torch.cuda.current_stream(dev).cuda_stream), "sdfr_pose_pair_errors")
    return degrees, distance


def pair_table(detections: dict, ground_truths: dict, groups: Optional[DetectionGroups] = None,
               symmetry_steps: int = 20):
    """(table (n_pairs,4) float64 on the device, groups): for every (detection, ground truth) pair of every group the
    row (iou, degrees, distance, key) with key = -iou; ``with_key(table, "pose")`` gives the pose matching's table.
    iou: ``box_iou`` of the ground truth's box against the detection's, paired mode, one call per distinct symmetry axis
    (the detection's box turned about its own axis in `symmetry_steps` steps, as ``metrics.iou_3d``), or the caller's
    ``detections["iou"]``.  degrees, distance: ``pose_pair_errors`` with the ground truth's symmetry axis."""
    dev = _device(detections, ground_truths)
    f64 = torch.float64
    if groups is None:
        groups = group_detections(detections["frame"], detections["class_id"], detections["score"],
                                  ground_truths["frame"], ground_truths["class_id"], dev)
    P, Ngt = groups.P, int(groups.gt_order.shape[0])
    dp, dq = _field(detections, "position", 3, f64, dev, P), _field(detections, "orientation", 4, f64, dev, P)
    gp, gq = _field(ground_truths, "position", 3, f64, dev, Ngt), _field(ground_truths, "orientation", 4, f64, dev, Ngt)
    sym = _field(ground_truths, "symmetry_axis", 0, torch.int32, dev, Ngt, default=-1)
    pd, pg = groups.pair_det, groups.pair_gt
    table = torch.empty((groups.n_pairs, 4), dtype=f64, device=dev)
    if groups.n_pairs == 0:
        return table, groups
    pair_sym = sym[pg]
    degrees, distance = pose_pair_errors(torch.cat([gp[pg], gq[pg]], 1), torch.cat([dp[pd], dq[pd]], 1), pair_sym)
    table[:, 1], table[:, 2] = degrees, distance
    if detections.get("iou") is not None:
        given = detections["iou"]
        given = given.detach() if isinstance(given, torch.Tensor) else torch.as_tensor(np.asarray(given))
        if tuple(given.shape) != (P, Ngt):
            raise ValueError(f"'iou': shape ({P},{Ngt}) expected (detections x ground truths), got {tuple(given.shape)}")
        table[:, 0] = given.to(device=dev, dtype=f64)[pd, pg]
    else:
        de, ge = _field(detections, "extents", 3, f64, dev, P), _field(ground_truths, "extents", 3, f64, dev, Ngt)
        for axis in torch.unique(pair_sym).tolist():
            if axis not in (-1, 0, 1, 2):
                raise ValueError(f"symmetry_axis={axis} must be -1, 0, 1 or 2")
            rows = torch.nonzero(pair_sym == axis)[:, 0]
            i, j = pd[rows], pg[rows]
            table[rows, 0] = box_iou(gp[j], gq[j], ge[j], dp[i], dq[i], de[i], paired=True,
                                     rotational_symmetry_axis=None if axis < 0 else axis, symmetry_steps=symmetry_steps)
    table[:, 3] = -table[:, 0]
    return table, groups


def with_key(table: torch.Tensor, key) -> torch.Tensor:
    """a copy of `table` whose key column is ``-iou`` ("iou"), ``degrees + 100 distance`` ("pose") or the given (n_pairs,)
    values"""
    out = table.clone()
    if isinstance(key, str):
        if key not in ("iou", "pose"):
            raise ValueError(f"key={key!r}: 'iou', 'pose' or a tensor expected")
        out[:, 3] = -table[:, 0] if key == "iou" else table[:, 1] + 100.0 * table[:, 2]
    else:
        out[:, 3] = key
    return out


def match_detections(table: torch.Tensor, groups: DetectionGroups, criteria) -> torch.Tensor:
    """matched (T,P) uint8 on the device: under criterion t (a row (iou_min, degrees_max, distance_max) of `criteria`)
    the LOCAL index of the ground truth the detection in column p took, or 255.  Columns are ``groups.det_order``.
    ``ValueError`` for a group with more than 64 ground truths (before the launch) or one the kernel refused."""
    dev = groups.device
    if groups.max_gt > MAX_GT:
        raise ValueError(f"a (frame, class) group has {groups.max_gt} ground truths: at most {MAX_GT} are supported")
    crit = (criteria.detach() if isinstance(criteria, torch.Tensor) else torch.as_tensor(np.asarray(criteria, np.float64)))
    crit = crit.to(device=dev, dtype=torch.float64).reshape(-1, 3).contiguous()
    if tuple(table.shape) != (groups.n_pairs, 4) or table.dtype != torch.float64 or not table.is_cuda:
        raise ValueError(f"table: a CUDA float64 tensor of shape ({groups.n_pairs},4) expected")
    table = table.contiguous()
    T = int(crit.shape[0])
    matched = torch.empty((T, groups.P), dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sdfr_ap_match(table.data_ptr(), groups.n_pairs, groups.pred_offset.data_ptr(),
                                            groups.gt_offset.data_ptr(), groups.pair_offset.data_ptr(), groups.G,
                                            groups.P, crit.data_ptr(), T, matched.data_ptr(), status.data_ptr(),
                                            dev.index, torch.cuda.current_stream(dev).cuda_stream), "sdfr_ap_match")
    if int(status.item()):
        raise ValueError("sdfr_ap_match refused a group (more than 64 ground truths, or offsets that disagree)")
    return matched


def average_precision(matched: torch.Tensor, groups: DetectionGroups) -> torch.Tensor:
    """ap (T,C) float64 on the device from matched (T,P): per criterion and class (``groups.classes``) the AP; NaN for
    a class without ground truths."""
    dev = groups.device
    if matched.dim() != 2 or matched.shape[1] != groups.P or matched.dtype != torch.uint8 or not matched.is_cuda:
        raise ValueError(f"matched: a CUDA uint8 tensor of shape (T,{groups.P}) expected")
    matched = matched.contiguous()
    T = int(matched.shape[0])
    ap = torch.empty((T, groups.C), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sdfr_ap_integrate(matched.data_ptr(), T, groups.P, groups.order.data_ptr(),
                                                groups.class_offset.data_ptr(), groups.n_gt.data_ptr(), groups.C,
                                                ap.data_ptr(), dev.index, torch.cuda.current_stream(dev).cuda_stream),
                   "sdfr_ap_integrate")
    return ap


def _mean_over_classes(ap: torch.Tensor) -> torch.Tensor:
    """(T,) from (T,C): the mean over the classes whose AP is not NaN; NaN where every class is"""
    ok = ~torch.isnan(ap)
    count = ok.sum(1)
    total = torch.where(ok, ap, torch.zeros_like(ap)).sum(1)
    return torch.where(count > 0, total / count.clamp(min=1), torch.full_like(total, float("nan")))


def _input_matches(matched: torch.Tensor, groups: DetectionGroups) -> np.ndarray:
    """(T,Nd) int64: per detection in INPUT order the INPUT index of the ground truth it took, or -1"""
    taken = matched != UNMATCHED
    where = (groups.gt_offset.to(torch.int64)[groups.column_group][None] + matched.to(torch.int64)).clamp(
        max=max(int(groups.gt_order.shape[0]) - 1, 0))
    found = groups.gt_order[where] if groups.gt_order.numel() else torch.zeros_like(where)
    out = torch.empty_like(where)
    out[:, groups.det_order] = torch.where(taken, found, torch.full_like(where, -1))
    return out.cpu().numpy()


def mean_average_precision(detections: dict, ground_truths: dict, iou_thresholds: Sequence[float],
                           degree_thresholds: Sequence[float], distance_thresholds: Sequence[float],
                           iou_min_for_pose: Optional[float] = None, symmetry_steps: int = 20,
                           return_matches: bool = False) -> Dict[str, np.ndarray]:
    """AP per class and its mean over IoU thresholds and over (degrees, distance) thresholds.

    IoU criteria ``(t, inf, inf)`` with key ``-iou`` for t in `iou_thresholds`; pose criteria ``(iou_min_for_pose or
    -inf, d, s)`` with key ``degrees + 100 distance`` for d in `degree_thresholds` (degrees), s in `distance_thresholds`
    (metres).  Returns numpy arrays: ``classes`` (C,) the sorted class ids, ``iou_ap`` (C,Ti), ``pose_ap`` (C,D,S),
    ``iou_map`` (Ti,), ``pose_map`` (D,S) (means over the classes that have ground truths), ``n_gt``, ``n_detections``
    (C,); with `return_matches` also ``iou_matched`` (Ti,Nd) and ``pose_matched`` (D S,Nd): per detection in input
    order the input index of the ground truth it took, or -1.  ``ValueError`` for a (frame, class) group with more than
    64 ground truths.  With distinct scores the result does not depend on the order of the frames, bit for bit."""
    dev = _device(detections, ground_truths)
    iou_t = [float(t) for t in iou_thresholds]
    deg_t, dist_t = [float(t) for t in degree_thresholds], [float(t) for t in distance_thresholds]
    groups = group_detections(detections["frame"], detections["class_id"], detections["score"],
                              ground_truths["frame"], ground_truths["class_id"], dev)
    if groups.max_gt > MAX_GT:
        raise ValueError(f"a (frame, class) group has {groups.max_gt} ground truths: at most {MAX_GT} are supported")
    table, _ = pair_table(detections, ground_truths, groups, symmetry_steps)
    inf = float("inf")
    lo = -inf if iou_min_for_pose is None else float(iou_min_for_pose)
    iou_criteria = np.array([(t, inf, inf) for t in iou_t], np.float64).reshape(-1, 3)
    pose_criteria = np.array([(lo, d, s) for d in deg_t for s in dist_t], np.float64).reshape(-1, 3)
    iou_matched = match_detections(table, groups, iou_criteria)
    pose_matched = match_detections(with_key(table, "pose"), groups, pose_criteria)
    iou_ap, pose_ap = average_precision(iou_matched, groups), average_precision(pose_matched, groups)
    C, D, S = groups.C, len(deg_t), len(dist_t)
    host = torch.cat([iou_ap.flatten(), _mean_over_classes(iou_ap), pose_ap.flatten(), _mean_over_classes(pose_ap)]).cpu().numpy()
    Ti, Tp = len(iou_t), D * S
    out = {"classes": groups.classes.cpu().numpy(),
           "iou_ap": host[:Ti * C].reshape(Ti, C).T.copy(),
           "iou_map": host[Ti * C:Ti * C + Ti].copy(),
           "pose_ap": host[Ti * C + Ti:Ti * C + Ti + Tp * C].reshape(Tp, C).T.reshape(C, D, S).copy(),
           "pose_map": host[Ti * C + Ti + Tp * C:].reshape(D, S).copy(),
           "n_gt": groups.n_gt.cpu().numpy().astype(np.int64),
           "n_detections": groups.n_detections.cpu().numpy().astype(np.int64)}
    if return_matches:
        out["iou_matched"] = _input_matches(iou_matched, groups)
        out["pose_matched"] = _input_matches(pose_matched, groups)
    return out
