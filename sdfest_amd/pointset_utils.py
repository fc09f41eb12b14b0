"""Point set helpers of the reference's ``sdfest/initialization/pointset_utils.py``: ``normalize_points`` (:12-31),
``depth_to_pointcloud`` with a mask and either camera convention (:34-89) over the depth kernels
(``sdfr_depth_count`` / ``sdfr_depth_to_points``), and the three ``change_*_camera_convention`` functions (:92-188)."""
from typing import Optional

import torch

from .differentiable_renderer import Camera
from .pipeline import quaternion_multiply

_CONVENTIONS = ("opengl", "opencv")


def normalize_points(points: torch.Tensor) -> tuple:
    """(points - centroid, centroid) along the second last dimension: (N,M,D) or (M,D) point sets."""
    centroids = torch.mean(points, dim=-2, keepdim=True)
    return points - centroids, centroids.squeeze()


def depth_to_pointcloud(depth_image: torch.Tensor, camera: Camera, normalize: bool = False,
                        mask: Optional[torch.Tensor] = None, convention: str = "opengl") -> torch.Tensor:
    """(H,W) float32 CUDA depth image -> (N,3) points of the pixels with ``depth * mask != 0`` (all non-zero pixels
    without a mask), row-major, in the camera frame of `convention`: "opengl" (x right, y up, z back) or "opencv"
    (x right, y down, z forward).  The OpenCV points are the OpenGL points with y and z negated, which is exact."""
    if convention not in _CONVENTIONS:
        raise ValueError(f"Unsupported camera convention {convention}.")
    if not (depth_image.is_cuda and depth_image.dtype == torch.float32 and depth_image.dim() == 2):
        raise RuntimeError("depth_image must be a float32 CUDA tensor of shape (H, W)")
    from .generated_views import depth_to_pointsets
    depth = depth_image if mask is None else depth_image * mask.to(depth_image.device)
    points = depth_to_pointsets(depth[None], camera)[0]
    if convention == "opencv":
        points = points * points.new_tensor([1.0, -1.0, -1.0])
    if normalize:
        points, _ = normalize_points(points)
    return points


def _check(in_convention: str, out_convention: str) -> None:
    if in_convention not in _CONVENTIONS:
        raise ValueError(f"In camera convention {in_convention} not supported.")
    if out_convention not in _CONVENTIONS:
        raise ValueError(f"Out camera convention {out_convention} not supported.")


def change_transform_camera_convention(in_transform: torch.Tensor, in_convention: str,
                                       out_convention: str) -> torch.Tensor:
    """Transform(s) (...,4,4) from a frame A to the in_convention camera frame -> to the out_convention camera frame."""
    _check(in_convention, out_convention)
    if in_convention == out_convention:
        return in_transform
    return torch.diag(in_transform.new_tensor([1.0, -1.0, -1.0, 1.0])) @ in_transform   # gl2cv == cv2gl


def change_position_camera_convention(in_position: torch.Tensor, in_convention: str,
                                      out_convention: str) -> torch.Tensor:
    """Position(s) (...,3) in the in_convention camera frame -> in the out_convention camera frame."""
    _check(in_convention, out_convention)
    if in_convention == out_convention:
        return in_position
    return in_position.new_tensor([1.0, -1.0, -1.0]) * in_position


def change_orientation_camera_convention(in_orientation_q: torch.Tensor, in_convention: str,
                                         out_convention: str) -> torch.Tensor:
    """Scalar-last quaternion(s) (...,4) rotating from a frame A to the in_convention camera frame -> to the
    out_convention camera frame (a rotation by 180 degrees about x in front)."""
    _check(in_convention, out_convention)
    if in_convention == out_convention:
        return in_orientation_q
    return quaternion_multiply(in_orientation_q.new_tensor([1.0, 0, 0, 0]), in_orientation_q)
