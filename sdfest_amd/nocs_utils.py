"""Similarity transforms from NOCS correspondences on the GPU: the reference's
``sdfest/initialization/datasets/nocs_utils.py`` (``estimate_similarity_transform``: 100 RANSAC hypotheses of five
correspondences each, Umeyama, a final fit over the inliers) over ``sdfr_similarity_ransac``, and the front half of
``NOCSDataset._estimate_object`` (nocs_dataset.py:673-698) over ``sdfr_nocs_count`` / ``sdfr_nocs_correspondences``.

All arithmetic of the fit is fp64 on the device.  The five indices of every hypothesis are an input of the kernel: by
default they are drawn on the device from ``seed`` (``sdfr_nocs_sample_indices``, a Philox stream of this project's
own -- numpy's global stream, which the reference draws from, is not reproduced), or the caller passes them.
"""
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib

N_ITERATIONS = _lib.ABI["SDFR_NOCS_HYPOTHESES"]
STATUS_OK = _lib.ABI["SDFR_NOCS_OK"]
STATUS_NONE = _lib.ABI["SDFR_NOCS_NONE"]
STATUS_POSE_ERROR = _lib.ABI["SDFR_NOCS_POSE_ERROR"]
STATUS_NAN_INPUT = _lib.ABI["SDFR_NOCS_NAN_INPUT"]
STATUS_TRUNCATED = _lib.ABI["SDFR_NOCS_TRUNCATED"]
MIN_CORRESPONDENCES = 30     # nocs_dataset.py:692
MAX_DEPTH = 32.0             # nocs_dataset.py:696


class PoseEstimationError(Exception):
    """Error if pose estimation encountered an error."""


class SimilarityTransforms(NamedTuple):
    """Device tensors of K fits: position (K,3), rotation_matrix (K,3,3), scale (K,), transform (K,4,4) float64 (NaN
    unless status is STATUS_OK); inlier_ratio (K,) float64; status, best_iteration, iterations_run (K,) int32;
    inlier_mask (total,) uint8 or None."""
    position: torch.Tensor
    rotation_matrix: torch.Tensor
    scale: torch.Tensor
    transform: torch.Tensor
    inlier_ratio: torch.Tensor
    status: torch.Tensor
    best_iteration: torch.Tensor
    iterations_run: torch.Tensor
    inlier_mask: Optional[torch.Tensor]


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def draw_sample_indices(offsets: torch.Tensor, seed: int = 0, object_seeds: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(K, 100, 5) int32: five distinct indices in [0, N_k) per hypothesis, from the object's seed (``object_seeds``
    (K,) int64 on the device, or ``seed`` for every object).  The place in the batch is not part of the stream."""
    K = offsets.numel() - 1
    dev = offsets.device
    out = torch.empty((K, N_ITERATIONS, 5), dtype=torch.int32, device=dev)
    if object_seeds is not None:
        object_seeds = object_seeds.to(device=dev, dtype=torch.int64).contiguous()
        if object_seeds.numel() != K:
            raise ValueError(f"object_seeds has {object_seeds.numel()} entries for {K} objects")
    _lib.check(_lib.lib().sdfr_nocs_sample_indices(offsets.data_ptr(), K, int(seed) & (2 ** 64 - 1),
                                                   object_seeds.data_ptr() if object_seeds is not None else None,
                                                   out.data_ptr(), dev.index, _stream(dev)),
               "sdfr_nocs_sample_indices")
    return out


def estimate_similarity_transforms(sources: torch.Tensor, targets: torch.Tensor, offsets, *, max_points: int = None,
                                   sample_indices: Optional[torch.Tensor] = None, seed: int = 0,
                                   object_seeds: Optional[torch.Tensor] = None,
                                   with_inlier_mask: bool = False) -> SimilarityTransforms:
    """``estimate_similarity_transform`` for K correspondence sets in one launch sequence; nothing is read back.

    sources, targets: (total, 3) CUDA tensors, both float32 or both float64; object k owns rows
    offsets[k] ... offsets[k + 1] - 1.  offsets: (K + 1,) int64, a device tensor or a host sequence.  max_points: an
    upper bound of the largest set (sizes the grid; needed when offsets is a device tensor, else taken from it); a set
    with more points than that is not fitted, its status is STATUS_TRUNCATED.  offsets must be non-decreasing.
    sample_indices: (K, 100, 5) int32 on the device; default: drawn there from seed / object_seeds."""
    if not (sources.is_cuda and targets.is_cuda and sources.dtype == targets.dtype
            and sources.dtype in (torch.float32, torch.float64)):
        raise RuntimeError("sources and targets must be CUDA tensors, both float32 or both float64")
    if sources.shape != targets.shape or sources.dim() != 2 or sources.shape[1] != 3:
        raise RuntimeError(f"sources {tuple(sources.shape)} and targets {tuple(targets.shape)} must both be (total, 3)")
    dev = sources.device
    sources, targets = sources.contiguous(), targets.contiguous()
    total = sources.shape[0]
    if not isinstance(offsets, torch.Tensor):
        host = [int(o) for o in offsets]
        if max_points is None:
            max_points = max((b - a for a, b in zip(host[:-1], host[1:])), default=0)
        offsets = torch.tensor(host, dtype=torch.int64, device=dev)
    elif max_points is None:
        raise ValueError("max_points is required when offsets is a device tensor")
    offsets = offsets.to(device=dev, dtype=torch.int64).contiguous()
    K = offsets.numel() - 1
    max_points = min(int(max_points), total)
    if sample_indices is None:
        sample_indices = draw_sample_indices(offsets, seed, object_seeds)
    sample_indices = sample_indices.to(device=dev, dtype=torch.int32).contiguous()
    if tuple(sample_indices.shape) != (K, N_ITERATIONS, 5):
        raise ValueError(f"sample_indices must be ({K}, {N_ITERATIONS}, 5), got {tuple(sample_indices.shape)}")
    L = _lib.lib()
    ws = _lib.workspace(L.sdfr_similarity_ransac_workspace_bytes(K, total, max_points),
                        "sdfr_similarity_ransac_workspace_bytes", dev)
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    r = SimilarityTransforms(torch.empty((K, 3), **f64), torch.empty((K, 3, 3), **f64), torch.empty((K,), **f64),
                             torch.empty((K, 4, 4), **f64), torch.empty((K,), **f64), torch.empty((K,), **i32),
                             torch.empty((K,), **i32), torch.empty((K,), **i32),
                             torch.empty((total,), dtype=torch.uint8, device=dev) if with_inlier_mask else None)
    dtype = _lib.ABI["SDFR_NOCS_F32"] if sources.dtype == torch.float32 else _lib.ABI["SDFR_NOCS_F64"]
    _lib.check(L.sdfr_similarity_ransac(sources.data_ptr(), targets.data_ptr(), dtype, offsets.data_ptr(), total,
                                        max_points, K, sample_indices.data_ptr(), r.position.data_ptr(),
                                        r.rotation_matrix.data_ptr(), r.scale.data_ptr(), r.transform.data_ptr(),
                                        r.inlier_ratio.data_ptr(), r.best_iteration.data_ptr(),
                                        r.iterations_run.data_ptr(), r.status.data_ptr(),
                                        r.inlier_mask.data_ptr() if with_inlier_mask else None, ws.data_ptr(),
                                        ws.numel(), dev.index, _stream(dev)), "sdfr_similarity_ransac")
    return r


def result_from_status(status: int, position, rotation_matrix, scale, transform) -> tuple:
    """The reference's return convention for one fit read back from the device: the four results, four ``None``, or
    the exception it raises."""
    if status == STATUS_POSE_ERROR:
        raise PoseEstimationError()
    if status == STATUS_NAN_INPUT:
        raise RuntimeError("There are NANs in the input.")
    if status == STATUS_NONE:
        return None, None, None, None
    if status == STATUS_TRUNCATED:
        raise ValueError("the set has more points than the fit's max_points")
    return np.asarray(position), np.asarray(rotation_matrix), float(scale), np.asarray(transform)


def estimate_similarity_transform(source, target, verbose: bool = False, *, sample_indices=None,
                                  seed: int = 0, device="cuda") -> tuple:
    """Similarity transform source -> target from point correspondences, RANSAC for robustness: the reference's
    function (nocs_utils.py:14-86) and return values -- ``(position (3,), rotation_matrix (3,3), scale,
    transform (4,4))`` as numpy float64 with ``transform @ source = scale * rotation_matrix @ source + position``, or
    four ``None`` (fewer than five correspondences, or an inlier ratio below 0.1).  Raises ``PoseEstimationError``
    where the reference does.

    source, target: (N,3) numpy arrays or tensors, float32 or float64 (anything else is converted to float64).
    sample_indices: (100, 5) indices of the hypotheses' correspondences; default: drawn on the device from ``seed``."""
    def prepare(x):
        x = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x))
        return x if x.dtype in (torch.float32, torch.float64) else x.double()
    s, t = prepare(source), prepare(target)
    if s.dtype != t.dtype:
        s, t = s.double(), t.double()
    if len(s) < 5 or len(t) < 5:
        print("Pose estimation failed. Not enough point correspondences: ", len(s))
        return None, None, None, None
    dev = s.device if s.is_cuda else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    s, t = s.to(dev).reshape(-1, 3), t.to(dev).reshape(-1, 3)
    if sample_indices is not None:
        sample_indices = torch.as_tensor(np.asarray(sample_indices), dtype=torch.int32).to(dev).reshape(1, N_ITERATIONS, 5)
    r = estimate_similarity_transforms(s, t, [0, len(s)], sample_indices=sample_indices, seed=seed)
    status = int(r.status.item())
    if verbose:
        print("BestInlierRatio:", r.inlier_ratio.item(), "iterations:", r.iterations_run.item())
    if status == STATUS_POSE_ERROR:
        print("Pose estimation failed: 0 variance in sampled points.")
    if status == STATUS_NONE:
        print("Pose estimation failed. Small inlier ratio: ", r.inlier_ratio.item())
    return result_from_status(status, r.position[0].cpu().numpy(), r.rotation_matrix[0].cpu().numpy(),
                              r.scale[0].item(), r.transform[0].cpu().numpy())


class Correspondences(NamedTuple):
    """source, target (total,3) float32 on the device; offsets (K+1,) int64 on the device; counts: host list;
    max_depth: host list (the largest valid depth per object)."""
    source: torch.Tensor
    target: torch.Tensor
    offsets: torch.Tensor
    counts: list
    max_depth: list


def nocs_correspondences(depth: torch.Tensor, mask: torch.Tensor, nocs_map: torch.Tensor, mask_ids: Sequence[int],
                         camera) -> Correspondences:
    """The correspondences of the K objects ``mask_ids`` of one frame (nocs_dataset.py:673-689): per object, the pixels
    with ``(mask == id) * depth != 0`` in row-major order; source = the NOCS colour (/ 255, z flipped, - 0.5), target
    = the OpenCV-frame back-projection.  depth (H,W) float32 metres, mask (H,W) uint8, nocs_map (H,W,3|4) uint8, all
    on the device; camera: a ``Camera``.  One read-back: the counts and the largest depths (the caller sizes the
    output by them and applies the reference's two rejections)."""
    dev = depth.device
    if not (depth.is_cuda and depth.dtype == torch.float32 and mask.dtype == torch.uint8
            and nocs_map.dtype == torch.uint8):
        raise RuntimeError("depth must be a float32 CUDA tensor, mask and nocs_map uint8")
    H, W = depth.shape
    if tuple(mask.shape) != (H, W) or nocs_map.dim() != 3 or tuple(nocs_map.shape[:2]) != (H, W):
        raise RuntimeError("mask and nocs_map must have the depth image's height and width")
    depth, mask, nocs_map = depth.contiguous(), mask.to(dev).contiguous(), nocs_map.to(dev).contiguous()
    K = len(mask_ids)
    ids = torch.tensor(list(mask_ids), dtype=torch.int32, device=dev)
    fx, fy, cx, cy, _ = camera.get_pinhole_camera_parameters(0.0)
    L = _lib.lib()
    ws = _lib.workspace(L.sdfr_nocs_workspace_bytes(W, H, K), "sdfr_nocs_workspace_bytes", dev)
    stats = torch.empty((2, max(K, 1)), dtype=torch.int32, device=dev)    # counts | max depth (as float bits)
    _lib.check(L.sdfr_nocs_count(depth.data_ptr(), mask.data_ptr(), W, H, ids.data_ptr(), K, stats[0].data_ptr(),
                                 stats[1].data_ptr(), ws.data_ptr(), ws.numel(), dev.index, _stream(dev)),
               "sdfr_nocs_count")
    host = stats.cpu()
    counts = host[0, :K].tolist()
    max_depth = host[1, :K].view(torch.float32).tolist()
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(off[-1])
    offsets = torch.tensor(off, dtype=torch.int64, device=dev)
    source = torch.empty((total, 3), dtype=torch.float32, device=dev)
    target = torch.empty((total, 3), dtype=torch.float32, device=dev)
    _lib.check(L.sdfr_nocs_correspondences(depth.data_ptr(), mask.data_ptr(), nocs_map.data_ptr(), nocs_map.shape[2],
                                           W, H, 1.0 / fx, 1.0 / fy, cx, cy, ids.data_ptr(), K, offsets.data_ptr(),
                                           total, ws.data_ptr(), source.data_ptr(), target.data_ptr(), dev.index,
                                           _stream(dev)), "sdfr_nocs_correspondences")
    return Correspondences(source, target, offsets, counts, max_depth)
