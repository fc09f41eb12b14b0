"""Reconstruction metrics on the GPU: the functions of the reference's ``sdfest/estimation/metrics.py`` with its names,
signatures, defaults and return conventions, over exact brute-force neighbour search (``sdfr_nn_query`` /
``sdfr_nn_reduce``, csrc/metrics.hip) instead of scipy's ``KDTree``.

Point sets may be numpy arrays or torch tensors on any device; they are converted to CUDA float32 (float64 inputs are
rounded), and a Python ``float`` is returned.  The distances are decided in float32 and the chosen pair's distance is
recomputed in float64; means, threshold ratios and F-scores follow the reference's formulas (strict ``<``; normalised
metrics divide by the extent first, then compare).  Every call is O(N M) work on the device; one pair of 20 000-point
sets takes well under a millisecond.

``reconstruction_metrics`` scores K pairs at once (one nearest pass per direction, one host read-back) and
``evaluate_metrics`` runs the ``metrics:`` mapping of an evaluation config with the passes shared between metrics.
Empty or non-finite point sets raise ``ValueError``.
"""
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .ap import mean_average_precision

__all__ = ["mean_accuracy", "mean_completeness", "symmetric_chamfer", "accuracy_thresh", "completeness_thresh",
           "reconstruction_fscore", "extent", "correct_thresh", "iou_3d", "mean_average_precision", "reconstruction_metrics", "evaluate_metrics", "nearest_neighbors"]

_MAX_T = _lib.ABI["SDFR_NN_MAX_THRESHOLDS"]
_STATS = _lib.ABI["SDFR_NN_STATS"]   # sum, max, count, NaN count, _MAX_T counts, _MAX_T normalised counts
PointSet = Union[np.ndarray, torch.Tensor]


def _device(sets) -> torch.device:
    for s in sets:
        if isinstance(s, torch.Tensor) and s.is_cuda:
            return s.device
    return torch.device("cuda", torch.cuda.current_device())


def _points(x, dev: torch.device, what: str) -> torch.Tensor:
    t = x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: (N,3) points expected, got shape {tuple(t.shape)}")
    if t.shape[0] == 0:
        raise ValueError(f"{what}: empty point set")
    return t.to(device=dev, dtype=torch.float32).contiguous()


def _pack(sets: List[torch.Tensor], dev: torch.device):
    """concatenated points, device int64 offsets [K + 1], host sizes"""
    sizes = np.array([s.shape[0] for s in sets], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    off_d = torch.from_numpy(off).pin_memory().to(dev, non_blocking=True)
    pts = sets[0] if len(sets) == 1 else torch.cat(sets)
    return pts, off_d, sizes


def _nn(q, qoff, qsizes, r, roff, rsizes, p: float, farthest: bool, dev: torch.device, index=None) -> torch.Tensor:
    """per query the distance (fp64) to its nearest (farthest) point of its pair's reference set (and its index into
    `index`, an int32 tensor, if given)"""
    L = _lib.lib()
    K, total_q, total_r = len(qsizes), int(q.shape[0]), int(r.shape[0])
    max_q, max_r = int(qsizes.max()), int(rsizes.max())
    ws = _lib.workspace(L.sdfr_nn_workspace_bytes(K, total_q, max_q), "sdfr_nn_workspace_bytes", dev)
    dist = torch.empty(total_q, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _lib.check(L.sdfr_nn_query(q.data_ptr(), qoff.data_ptr(), total_q, max_q, r.data_ptr(), roff.data_ptr(),
                                   total_r, max_r, K, float(p), int(farthest), dist.data_ptr(),
                                   index.data_ptr() if index is not None else None, ws.data_ptr(),
                                   ws.numel(), dev.index, stream), "sdfr_nn_query")
    return dist


def _reduce(dist, off, K: int, thresholds: Sequence[float], extent_d: Optional[torch.Tensor],
            dev: torch.device) -> torch.Tensor:
    """(K, 4 + 2 T) device fp64: sum, max, count, NaN count, then T counts below the thresholds, then T normalised"""
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    chunks = [list(thresholds[i:i + _MAX_T]) for i in range(0, len(thresholds), _MAX_T)] or [[]]
    outs = []
    for ch in chunks:
        st = torch.empty((K, _STATS), dtype=torch.float64, device=dev)
        h = (np.array(ch + [0.0] * (_MAX_T - len(ch)), dtype=np.float64))
        with torch.cuda.device(dev):
            _lib.check(L.sdfr_nn_reduce(dist.data_ptr(), off.data_ptr(), int(dist.shape[0]), K,
                                        h.ctypes.data, len(ch), extent_d.data_ptr() if extent_d is not None else None,
                                        st.data_ptr(), dev.index, stream), "sdfr_nn_reduce")
        outs.append(st[:, 4:4 + len(ch)])
        outs.append(st[:, 4 + _MAX_T:4 + _MAX_T + len(ch)])
        base = st[:, :4]
    T = len(thresholds)
    cnt = torch.cat(outs[0::2], 1) if T else base[:, :0]
    cntn = torch.cat(outs[1::2], 1) if T else base[:, :0]
    return torch.cat([base, cnt, cntn], 1)


class _Passes:
    """host results of the passes for K pairs (gt k, rec k): one read-back"""

    def __init__(self, gt: List[PointSet], rec: List[PointSet], p_norm, thresholds: Sequence[float],
                 normalize: bool, need_acc: bool = True, need_comp: bool = True) -> None:
        p = float(p_norm)
        if not p >= 1.0:
            raise ValueError(f"p_norm={p_norm}: the Minkowski p-norm needs p >= 1")
        if len(gt) != len(rec) or not gt:
            raise ValueError(f"{len(gt)} ground-truth and {len(rec)} reconstructed point sets: equal, nonzero counts "
                             "expected")
        dev = _device(list(gt) + list(rec))
        g = [_points(x, dev, f"points_gt[{k}]") for k, x in enumerate(gt)]
        r = [_points(x, dev, f"points_rec[{k}]") for k, x in enumerate(rec)]
        K = len(g)
        gp, goff, gs = _pack(g, dev)
        rp, roff, rs = _pack(r, dev)
        self.K, self.n_gt, self.n_rec, self.thresholds = K, gs, rs, [float(t) for t in thresholds]
        T = len(self.thresholds)
        bad = (~torch.isfinite(gp)).any() | (~torch.isfinite(rp)).any()
        parts = []
        ext_d = None
        if normalize:   # extent of every gt set: max over its points of the farthest point (Euclidean)
            far = _nn(gp, goff, gs, gp, goff, gs, 2.0, True, dev)
            ext_d = _reduce(far, goff, K, [], None, dev)[:, 1].contiguous()
            parts.append(ext_d)
        if need_acc:    # rec -> gt
            parts.append(_reduce(_nn(rp, roff, rs, gp, goff, gs, p, False, dev), roff, K, self.thresholds, ext_d,
                                 dev).flatten())
        if need_comp:   # gt -> rec
            parts.append(_reduce(_nn(gp, goff, gs, rp, roff, rs, p, False, dev), goff, K, self.thresholds, ext_d,
                                 dev).flatten())
        parts.append(bad.to(torch.float64).reshape(1))
        h = torch.cat(parts).cpu().numpy()   # the one host synchronisation
        if h[-1] != 0:
            raise ValueError("point sets must be finite (NaN or inf found)")
        i = 0
        self.extent = None
        if normalize:
            self.extent, i = h[:K], K
        W = 4 + 2 * T
        self.acc = self.comp = None
        if need_acc:
            self.acc, i = h[i:i + K * W].reshape(K, W), i + K * W
        if need_comp:
            self.comp, i = h[i:i + K * W].reshape(K, W), i + K * W

    # per pair k, the reference's formulas
    def mean(self, which: str, k: int, normalize: bool) -> float:
        s = self.acc if which == "acc" else self.comp
        n = self.n_rec[k] if which == "acc" else self.n_gt[k]
        m = float(s[k, 0]) / float(n)
        return m / self.extent[k] if normalize else m

    def ratio(self, which: str, k: int, threshold: float, normalize: bool) -> float:
        s = self.acc if which == "acc" else self.comp
        n = self.n_rec[k] if which == "acc" else self.n_gt[k]
        j = self.thresholds.index(float(threshold))
        T = len(self.thresholds)
        return float(s[k, 4 + T * int(normalize) + j]) / float(n)

    def chamfer(self, k: int, normalize: bool) -> float:
        return (self.mean("comp", k, normalize) + self.mean("acc", k, normalize)) / 2

    def fscore(self, k: int, threshold: float, normalize: bool):
        recall = self.ratio("comp", k, threshold, normalize)
        precision = self.ratio("acc", k, threshold, normalize)
        if recall < 1e-7 or precision < 1e-7:
            return 0
        return 2 / (1 / recall + 1 / precision)


def mean_accuracy(points_gt: PointSet, points_rec: PointSet, p_norm: int = 2, normalize: bool = False) -> float:
    """Mean p-norm distance from each reconstructed point to its closest ground-truth point (the asymmetric chamfer
    distance rec -> gt); with `normalize`, divided by ``extent(points_gt)``.  O(N M) on the GPU."""
    return _Passes([points_gt], [points_rec], p_norm, [], normalize, need_comp=False).mean("acc", 0, normalize)


def mean_completeness(points_gt: PointSet, points_rec: PointSet, p_norm: int = 2, normalize: bool = False) -> float:
    """Mean p-norm distance from each ground-truth point to its closest reconstructed point (gt -> rec); with
    `normalize`, divided by ``extent(points_gt)``.  O(N M) on the GPU."""
    return _Passes([points_gt], [points_rec], p_norm, [], normalize, need_acc=False).mean("comp", 0, normalize)


def symmetric_chamfer(points_gt: PointSet, points_rec: PointSet, p_norm: int = 2, normalize: bool = False) -> float:
    """(mean_completeness + mean_accuracy) / 2.  O(N M) on the GPU."""
    return _Passes([points_gt], [points_rec], p_norm, [], normalize).chamfer(0, normalize)


def completeness_thresh(points_gt: PointSet, points_rec: PointSet, threshold: float, p_norm: int = 2,
                        normalize: bool = False) -> float:
    """Ratio of ground-truth points whose closest reconstructed point is closer than `threshold` (strict; with
    `normalize` the distance is divided by ``extent(points_gt)`` first).  O(N M) on the GPU."""
    return _Passes([points_gt], [points_rec], p_norm, [threshold], normalize,
                   need_acc=False).ratio("comp", 0, threshold, normalize)


def accuracy_thresh(points_gt: PointSet, points_rec: PointSet, threshold: float, p_norm: int = 2,
                    normalize: bool = False) -> float:
    """Ratio of reconstructed points whose closest ground-truth point is closer than `threshold` (strict; with
    `normalize` the distance is divided by ``extent(points_gt)`` first).  O(N M) on the GPU."""
    return _Passes([points_gt], [points_rec], p_norm, [threshold], normalize,
                   need_comp=False).ratio("acc", 0, threshold, normalize)


def reconstruction_fscore(points_gt: PointSet, points_rec: PointSet, threshold: float, p_norm: int = 2,
                          normalize: bool = False) -> float:
    """Harmonic mean of precision (accuracy_thresh) and recall (completeness_thresh); the int 0 when either is below
    1e-7, as in the reference.  O(N M) on the GPU."""
    return _Passes([points_gt], [points_rec], p_norm, [threshold], normalize).fscore(0, threshold, normalize)


def extent(points: PointSet) -> float:
    """The largest Euclidean distance between two points of the set: the maximum over the points of the farthest
    point (exact, O(N^2) on the GPU; the reference's convex hull + distance matrix gives the same value)."""
    dev = _device([points])
    x = _points(points, dev, "points")
    xp, off, sz = _pack([x], dev)
    far = _nn(xp, off, sz, xp, off, sz, 2.0, True, dev)
    st = _reduce(far, off, 1, [], None, dev)
    bad = (~torch.isfinite(xp)).any().to(torch.float64).reshape(1)
    h = torch.cat([st[0, 1:2], bad]).cpu().numpy()
    if h[1] != 0:
        raise ValueError("point sets must be finite (NaN or inf found)")
    return float(h[0])


def nearest_neighbors(queries: PointSet, refs: PointSet, p_norm=2, farthest: bool = False):
    """For every query point its nearest (or farthest) point of `refs` in the Minkowski p-norm: (distance (N,) float64,
    index (N,) int32) CUDA tensors -- ``scipy.spatial.KDTree(refs).query(queries, p=p_norm)`` by brute force, O(N M).
    The float32 norm sum decides (ties go to the lowest index); the chosen pair's distance is float64."""
    p = float(p_norm)
    if not p >= 1.0:
        raise ValueError(f"p_norm={p_norm}: the Minkowski p-norm needs p >= 1")
    dev = _device([queries, refs])
    qp, qoff, qs = _pack([_points(queries, dev, "queries")], dev)
    rp, roff, rs = _pack([_points(refs, dev, "refs")], dev)
    index = torch.empty(qp.shape[0], dtype=torch.int32, device=dev)
    return _nn(qp, qoff, qs, rp, roff, rs, p, farthest, dev, index), index


# ---- poses ----------------------------------------------------------------------------------------------------------
class _Quat:
    """the part of scipy's ``Rotation`` that ``correct_thresh`` uses, for a scalar-last (x, y, z, w) quaternion"""

    def __init__(self, q) -> None:
        q = np.asarray(q.detach().cpu() if isinstance(q, torch.Tensor) else q, dtype=np.float64).reshape(4)
        self.q = q / np.linalg.norm(q)

    def as_quat(self) -> np.ndarray:
        return self.q.copy()

    def as_matrix(self) -> np.ndarray:
        x, y, z, w = self.q
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

    def apply(self, v) -> np.ndarray:
        return self.as_matrix() @ np.asarray(v, dtype=np.float64)

    def inv(self) -> "_Quat":
        return _Quat(np.array([-self.q[0], -self.q[1], -self.q[2], self.q[3]]))

    def __mul__(self, other: "_Quat") -> "_Quat":   # self after other (Hamilton product)
        x1, y1, z1, w1 = self.q
        x2, y2, z2, w2 = other.q
        return _Quat(np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                               w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2]))

    def magnitude(self) -> float:
        return 2.0 * np.arctan2(np.linalg.norm(self.q[:3]), abs(self.q[3]))


def _rotation(r):
    if all(hasattr(r, a) for a in ("apply", "inv", "magnitude")):
        return r
    return _Quat(r)


def iou_3d(position_gt, orientation_gt, extent_gt, position_prediction, orientation_prediction, extent_prediction,
           rotational_symmetry_axis: Optional[int] = None, symmetry_steps: int = 20) -> float:
    """The 3D IoU of the ground-truth and the predicted oriented bounding box (``boxes.box_iou`` for one pair, exact
    in float64 on the GPU): positions (3,), extents (3,) full side lengths, orientations as in ``correct_thresh``
    (scipy ``Rotation``-like objects or scalar-last quaternions).  rotational_symmetry_axis: the largest IoU over the
    prediction turned about its own axis in `symmetry_steps` equal steps."""
    from .boxes import box_iou
    quat = lambda r: r.as_quat() if hasattr(r, "as_quat") else r
    iou = box_iou(position_gt, quat(orientation_gt), extent_gt, position_prediction, quat(orientation_prediction),
                  extent_prediction, paired=True, rotational_symmetry_axis=rotational_symmetry_axis,
                  symmetry_steps=symmetry_steps)
    return float(iou[0])


def correct_thresh(position_gt, position_prediction, orientation_gt, orientation_prediction, extent_gt=None,
                   extent_prediction=None, points_gt=None, points_prediction=None,
                   position_threshold: Optional[float] = None, degree_threshold: Optional[float] = None,
                   iou_3d_threshold: Optional[float] = None, fscore_threshold: Optional[float] = None,
                   rotational_symmetry_axis: Optional[int] = None) -> int:
    """1 if the pose (and, with `fscore_threshold`, the reconstruction's F-score at 0.01) is within every given
    threshold, else 0.  Orientations are scipy ``Rotation`` objects (duck-typed: ``apply``, ``*``, ``inv``,
    ``magnitude``) or scalar-last quaternions.  `iou_3d_threshold` needs both `extent_gt` and `extent_prediction` (the
    boxes' full side lengths; ``iou_3d`` with `rotational_symmetry_axis` passed through); without them it raises
    ``NotImplementedError``, as the reference always does."""
    if position_threshold is not None:
        to_np = lambda v: np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
        position_error = np.linalg.norm(to_np(position_gt) - to_np(position_prediction))
        if position_error > position_threshold:
            return 0
    if degree_threshold is not None:
        rad_threshold = degree_threshold * np.pi / 180.0
        r_gt, r_pred = _rotation(orientation_gt), _rotation(orientation_prediction)
        if type(r_gt) is not type(r_pred):   # one scipy Rotation, one quaternion: compare as quaternions
            r_gt = r_gt if isinstance(r_gt, _Quat) else _Quat(r_gt.as_quat())
            r_pred = r_pred if isinstance(r_pred, _Quat) else _Quat(r_pred.as_quat())
        if rotational_symmetry_axis is not None:
            p = np.array([0.0, 0.0, 0.0])
            p[rotational_symmetry_axis] = 1.0
            p1 = r_gt.apply(p)
            p2 = r_pred.apply(p)
            rad_error = np.arccos(p1 @ p2)
        else:
            rad_error = (r_gt * r_pred.inv()).magnitude()
        if rad_error > rad_threshold:
            return 0
    if iou_3d_threshold is not None:
        if extent_gt is None or extent_prediction is None:
            raise NotImplementedError("3D IoU is not impemented yet. (without extent_gt and extent_prediction: the "
                                      "boxes' side lengths are needed)")
        if iou_3d(position_gt, orientation_gt, extent_gt, position_prediction, orientation_prediction,
                  extent_prediction, rotational_symmetry_axis) < iou_3d_threshold:
            return 0
    if fscore_threshold is not None:
        fscore = reconstruction_fscore(points_gt, points_prediction, 0.01)
        if fscore < fscore_threshold:
            return 0
    return 1


# ---- batches and configs --------------------------------------------------------------------------------------------
def _as_list(x) -> List[PointSet]:
    if isinstance(x, (list, tuple)):
        return list(x)
    if isinstance(x, (np.ndarray, torch.Tensor)) and x.ndim == 3:
        return [x[k] for k in range(x.shape[0])]
    raise ValueError("(K,N,3) points or a list of (N_k,3) point sets expected")


def reconstruction_metrics(points_gt, points_rec, thresholds: Iterable[float] = (0.01,), p_norm=2,
                           normalize: bool = False) -> Dict[str, torch.Tensor]:
    """All point metrics for K pairs (gt k, rec k) in one launch sequence and one host read-back.

    points_gt, points_rec: (K,N,3) / (K,M,3), or lists of K ragged (N_k,3) / (M_k,3) sets.  Returns (K,) float64
    tensors (on the CPU): ``accuracy``, ``completeness``, ``chamfer``, and per threshold t ``accuracy@t``,
    ``completeness@t``, ``fscore@t``; with `normalize` (all values as the reference's ``normalize=True``) also
    ``extent`` (of each gt set).  Entry k equals the single-pair functions on (gt k, rec k) exactly.  O(sum N_k M_k)."""
    th = [float(t) for t in thresholds]
    P = _Passes(_as_list(points_gt), _as_list(points_rec), p_norm, th, normalize)
    K = P.K
    col = lambda f: torch.tensor([float(f(k)) for k in range(K)], dtype=torch.float64)
    out = {"accuracy": col(lambda k: P.mean("acc", k, normalize)),
           "completeness": col(lambda k: P.mean("comp", k, normalize)),
           "chamfer": col(lambda k: P.chamfer(k, normalize))}
    for t in th:
        out[f"accuracy@{t:g}"] = col(lambda k: P.ratio("acc", k, t, normalize))
        out[f"completeness@{t:g}"] = col(lambda k: P.ratio("comp", k, t, normalize))
        out[f"fscore@{t:g}"] = col(lambda k: P.fscore(k, t, normalize))
    if normalize:
        out["extent"] = torch.tensor(P.extent, dtype=torch.float64)
    return out


_CONFIG_FUNCTIONS = {"mean_accuracy", "mean_completeness", "symmetric_chamfer", "accuracy_thresh",
                     "completeness_thresh", "reconstruction_fscore"}
_CONFIG_MODULES = {"sdfest.estimation.metrics", "sdfest_amd.metrics"}


def _config_entry(name: str, m) -> Tuple[str, dict]:
    f = m.get("f") if isinstance(m, dict) else None
    mod, _, fn = str(f).rpartition(".")
    if fn not in _CONFIG_FUNCTIONS or mod not in _CONFIG_MODULES:
        raise ValueError(f"metric {name!r}: unknown f={f!r} (supported: sdfest.estimation.metrics."
                         f"{{{', '.join(sorted(_CONFIG_FUNCTIONS))}}})")
    kw = dict(m.get("kwargs") or {})
    allowed = {"p_norm", "normalize"} | ({"threshold"} if fn.endswith(("_thresh", "_fscore")) else set())
    if set(kw) - allowed or (fn.endswith(("_thresh", "_fscore")) and "threshold" not in kw):
        raise ValueError(f"metric {name!r}: kwargs {sorted(kw)} do not fit {fn}")
    return fn, kw


def evaluate_metrics(points_gt: PointSet, points_rec: PointSet, metrics_config: dict) -> Dict[str, float]:
    """The ``metrics:`` mapping of an evaluation config ({name: {"f": "sdfest.estimation.metrics.X", "kwargs": {...}}},
    as loaded from YAML) on one pair: {name: float}, the values of calling each function, with one pass per
    direction (and one extent pass if any metric normalises) for each p-norm in the config."""
    entries = {name: _config_entry(name, m) for name, m in metrics_config.items()}
    groups: Dict[float, dict] = {}
    for fn, kw in entries.values():
        g = groups.setdefault(float(kw.get("p_norm", 2)), {"t": [], "normalize": False})
        if "threshold" in kw and float(kw["threshold"]) not in g["t"]:
            g["t"].append(float(kw["threshold"]))
        g["normalize"] |= bool(kw.get("normalize", False))
    passes = {p: _Passes([points_gt], [points_rec], p, g["t"], g["normalize"]) for p, g in groups.items()}
    out = {}
    for name, (fn, kw) in entries.items():
        P = passes[float(kw.get("p_norm", 2))]
        nz = bool(kw.get("normalize", False))
        if fn == "mean_accuracy":
            v = P.mean("acc", 0, nz)
        elif fn == "mean_completeness":
            v = P.mean("comp", 0, nz)
        elif fn == "symmetric_chamfer":
            v = P.chamfer(0, nz)
        elif fn == "accuracy_thresh":
            v = P.ratio("acc", 0, kw["threshold"], nz)
        elif fn == "completeness_thresh":
            v = P.ratio("comp", 0, kw["threshold"], nz)
        else:
            v = P.fscore(0, kw["threshold"], nz)
        out[name] = float(v)
    return out
