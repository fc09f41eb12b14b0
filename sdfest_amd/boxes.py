"""Oriented bounding boxes on the GPU (``sdfr_sdf_bounds`` / ``sdfr_box_iou``, csrc/boxes.hip).

``sdf_bounds`` gives the axis-aligned bounds of a decoded SDF's iso-surface in the SDF's normalised frame -- bitwise the
minimum and maximum of the vertices ``extract_mesh`` would return, without making the mesh -- and ``box_iou`` the exact
3D IoU of oriented boxes in float64, the metric the reference leaves as a TODO (sdfest/estimation/metrics.py:66-70).
A box is a centre (3,), an orientation (4,) (x, y, z, w) and its full side lengths (3,): the set c + R(q) x,
|x_i| <= e_i / 2.
"""
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

__all__ = ["sdf_bounds", "box_iou"]


def sdf_bounds(sdf: torch.Tensor, level: float, complete: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The bounds of the iso-surface of `sdf` at `level`: (lo (N,3), hi (N,3) float32, crossed (N,) int32) on the device,
    for sdf (R,R,R) (N = 1) or (N,R,R,R), CUDA float32, 2 <= R <= 256.  lo / hi are bitwise
    ``extract_mesh(sdf, level, complete).vertices.amin(0)`` / ``amax(0)`` and `crossed` is its vertex count; a grid the
    level does not cross has crossed = 0, lo = +inf, hi = -inf.  complete: as ``extract_mesh``.  Kernels on the current
    stream only, nothing read back."""
    if sdf.dim() == 3:
        sdf = sdf[None]
    if sdf.dim() != 4 or not (sdf.shape[1] == sdf.shape[2] == sdf.shape[3]):
        raise ValueError(f"sdf of shape {tuple(sdf.shape)}: (R,R,R) or (N,R,R,R) cubic grids expected")
    if not sdf.is_cuda or sdf.dtype != torch.float32:
        raise TypeError("sdf must be a CUDA float32 tensor (sdfest_amd has no CPU path)")
    N, R = int(sdf.shape[0]), int(sdf.shape[1])
    sdf = sdf.detach().contiguous()
    dev = sdf.device
    bounds = torch.empty((N, 6), dtype=torch.float32, device=dev)
    crossed = torch.empty((N,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sdfr_sdf_bounds(sdf.data_ptr(), N, R, 1 if complete else 0, float(np.float32(level)),
                                              bounds.data_ptr(), crossed.data_ptr(), dev.index,
                                              torch.cuda.current_stream(dev).cuda_stream), "sdfr_sdf_bounds")
    return bounds[:, :3], bounds[:, 3:], crossed


def _host_or_device(x):
    return x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))


def _pack_boxes(centers, orientations, extents, what: str):
    """the (K,10) rows of K boxes, still where they were given (shape errors come before any GPU work)"""
    parts = []
    for name, v, w in (("centers", centers, 3), ("orientations", orientations, 4), ("extents", extents, 3)):
        t = _host_or_device(v)
        if t.dim() == 1 and t.shape[0] == w:
            t = t[None]
        if t.dim() != 2 or t.shape[1] != w:
            raise ValueError(f"{name}_{what}: ({w},) or (K,{w}) expected, got shape {tuple(t.shape)}")
        if not (t.is_floating_point()):
            t = t.to(torch.float64)
        parts.append(t)
    if not (parts[0].shape[0] == parts[1].shape[0] == parts[2].shape[0]):
        raise ValueError(f"boxes {what}: {parts[0].shape[0]} centers, {parts[1].shape[0]} orientations and "
                         f"{parts[2].shape[0]} extents")
    return parts


def box_iou(centers_a, orientations_a, extents_a, centers_b, orientations_b, extents_b, paired: bool = False,
            rotational_symmetry_axis: Optional[int] = None, symmetry_steps: int = 20,
            return_intersection: bool = False):
    """The 3D IoU of oriented boxes, exact up to float64 rounding, on the GPU.

    centers (N,3), orientations (N,4) scalar-last (normalised inside), extents (N,3) full side lengths for the boxes a,
    and (M,...) for the boxes b (a single box may be given without its leading dimension); tensors or arrays of any
    float dtype, converted to float64 on the device.  Returns the (N,M) float64 matrix of every a against every b, or
    with `paired` (N == M) the (N,) IoUs of a_k against b_k; with `return_intersection` also the intersection volumes,
    same shape.  rotational_symmetry_axis 0 | 1 | 2: every box b is also turned about its own axis by 2 pi s /
    symmetry_steps and the largest IoU counts (a category whose turn about that axis cannot be observed).  A box with a
    non-finite entry, a non-positive extent or a zero quaternion gives NaN.  One launch, nothing read back."""
    a = _pack_boxes(centers_a, orientations_a, extents_a, "a")
    b = _pack_boxes(centers_b, orientations_b, extents_b, "b")
    N, M = int(a[0].shape[0]), int(b[0].shape[0])
    if paired and N != M:
        raise ValueError(f"paired: {N} boxes a and {M} boxes b")
    axis = -1 if rotational_symmetry_axis is None else int(rotational_symmetry_axis)
    steps = int(symmetry_steps)
    if axis not in (-1, 0, 1, 2):
        raise ValueError(f"rotational_symmetry_axis={rotational_symmetry_axis} must be None, 0, 1 or 2")
    if axis >= 0 and not 1 <= steps <= 65536:
        raise ValueError(f"symmetry_steps={symmetry_steps} must be in [1, 65536]")
    dev = next((t.device for t in a + b if t.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    rows = lambda parts: torch.cat([t.to(device=dev, dtype=torch.float64) for t in parts], 1).contiguous()
    ra, rb = rows(a), rows(b)
    shape = (N,) if paired else (N, M)
    iou = torch.empty(shape, dtype=torch.float64, device=dev)
    vol = torch.empty(shape, dtype=torch.float64, device=dev) if return_intersection else None
    abi = _lib.ABI
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sdfr_box_iou(ra.data_ptr(), N, rb.data_ptr(), M,
                                           abi["SDFR_BOX_IOU_PAIRED"] if paired else abi["SDFR_BOX_IOU_MATRIX"], axis,
                                           steps, iou.data_ptr(), None if vol is None else vol.data_ptr(), dev.index,
                                           torch.cuda.current_stream(dev).cuda_stream), "sdfr_box_iou")
    return (iou, vol) if return_intersection else iou
