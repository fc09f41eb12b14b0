"""Pose uncertainty: the Gauss-Newton information of the depth residual and what follows from it.

The estimation forms return a point estimate; this module says how well the observation determines it.  The normal
matrix J^T J of the depth residual (with J^T r, sum r^2 and the pixel count) comes from one HIP call over all views
(``sdfr_render_information``, include/sdfr.h group 14); the rest -- the change to seven local parameters, the sum over
an object's views, the eigen-decomposition and the covariance -- is 7 x 7 algebra in float64 torch and works on CPU
tensors as well.

Local parameters (the *tangent*): position (3, metres), a world-frame rotation vector w (3, radians,
``q <- exp(w / 2) (x) q``, quaternions scalar-last) and log-scale (1).  A direction of that space the depth image does
not constrain -- the spin of a bottle about its axis, any rotation of a sphere -- shows as a (numerically) zero
eigenvalue: ``pose_covariance`` reports it through ``rank`` and ``unobserved`` instead of inverting it.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from .differentiable_renderer import Camera, _check_inputs, _ptr, _stream, _workspace

GRAM_SIZE = 10   # (d0 .. d7, r, 1)


def render_information(depth: torch.Tensor, target: torch.Tensor, sdf: torch.Tensor, position: torch.Tensor,
                       orientation: torch.Tensor, inv_scale: torch.Tensor, camera: Camera,
                       inlier_threshold: float = 0.0, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,10,10) float64: per view the Gram matrix of f = (d depth / d (px,py,pz,qx,qy,qz,qw,inv_scale), depth - target, 1)
    over the pixels with depth > 0, target > 0 and -- for ``inlier_threshold`` > 0 -- |target - depth| / target below it.

    ``depth`` is the rendered estimate at the given pose ((H,W) or (B,H,W)), ``target`` the observation; the pose has
    the shapes ``render_depth_gpu`` / ``render_depth_batch`` take: position (3,) or (B,3), orientation (4,) or (B,4),
    inv_scale () or (B,); ``sdf`` (R,R,R) shared by the views or (B,R,R,R).  ``[:8,:8]`` is J^T J, ``[:8,8]`` J^T r,
    ``[8,8]`` sum r^2, ``[9,9]`` the pixel count.  Exactly symmetric, the same bits on every call."""
    _check_inputs((depth, "depth"), (target, "target"), (sdf, "sdf"), (position, "position"),
                  (orientation, "orientation"), (inv_scale, "inv_scale"))
    pos, quat, isc = position.reshape(-1, 3), orientation.reshape(-1, 4), inv_scale.reshape(-1)
    B = pos.shape[0]
    if quat.shape[0] != B or isc.shape[0] != B:
        raise RuntimeError("expected position (B,3), orientation (B,4), inv_scale (B,)")
    H, W = camera.height, camera.width
    if depth.numel() != B * H * W or target.numel() != B * H * W or tuple(depth.shape[-2:]) != (H, W):
        raise RuntimeError(f"expected depth and target of {B} x {H} x {W} pixels")
    R = sdf.shape[-1]
    if sdf.dim() == 3:
        stride = 0
    elif sdf.dim() == 4 and sdf.shape[0] == B:
        stride = R * R * R
    else:
        raise RuntimeError("sdf must be (R,R,R) or (B,R,R,R)")
    if tuple(sdf.shape[-3:]) != (R, R, R):
        raise RuntimeError("sdf must be cubic")
    fx, fy, cx, cy, _ = camera.get_pinhole_camera_parameters(0.5)
    dev = sdf.device
    L = _lib.lib()
    nbytes = L.sdfr_render_information_workspace_bytes(B, W, H)
    if workspace is None and nbytes:
        workspace = _workspace(dev, nbytes)   # (the renderer's per-stream scratch buffer)
    ws = _lib.workspace(nbytes, "sdfr_render_information_workspace_bytes", dev, workspace)
    gram = torch.empty((B, GRAM_SIZE, GRAM_SIZE), dtype=torch.float64, device=dev)
    rc = L.sdfr_render_information(_ptr(depth), _ptr(target), _ptr(sdf), R, stride, _ptr(pos), _ptr(quat), _ptr(isc),
                                   B, W, H, cx, cy, fx, fy, float(inlier_threshold), _ptr(gram), _ptr(ws), ws.numel(),
                                   dev.index, _stream(dev))
    _lib.check(rc, "sdfr_render_information")
    return gram


def _quaternion_multiply(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    ax, ay, az, aw = torch.unbind(a, -1)
    bx, by, bz, bw = torch.unbind(b, -1)
    return torch.stack((aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz), -1)


def _rotation_matrix(q: torch.Tensor) -> torch.Tensor:
    x, y, z, w = torch.unbind(q / torch.linalg.norm(q, dim=-1, keepdim=True), -1)
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), -1).reshape(q.shape[:-1] + (3, 3))


def tangent_map(orientation: torch.Tensor, inv_scale: torch.Tensor,
                camera_orientations: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,8,7) float64: d (px,py,pz,qx,qy,qz,qw,inv_scale) / d (position, rotation vector, log-scale) at the given
    pose.  Position: the identity.  Rotation: column k is half the quaternion product (e_k, 0) (x) q of the unit
    quaternion -- the derivative of ``exp(w / 2) (x) q`` at w = 0.  Log-scale: d inv_scale / d log(scale) = -inv_scale.
    With ``camera_orientations`` (B,4) -- the cameras' orientations in the world, as the pipelines take them -- the
    position and rotation columns are those of WORLD-frame steps (a world step d is the camera-frame step R_c^T d)."""
    q = orientation.to(torch.float64).reshape(-1, 4)
    isc = inv_scale.to(torch.float64).reshape(-1)
    B = q.shape[0]
    q = q / torch.linalg.norm(q, dim=-1, keepdim=True)
    T = q.new_zeros((B, 8, 7))
    T[:, 0, 0] = T[:, 1, 1] = T[:, 2, 2] = 1.0
    for k in range(3):
        e = q.new_zeros(4)
        e[k] = 1.0
        T[:, 3:7, 3 + k] = 0.5 * _quaternion_multiply(e.expand(B, 4), q)
    T[:, 7, 6] = -isc
    if camera_orientations is not None:
        M = _rotation_matrix(camera_orientations.to(torch.float64).reshape(-1, 4)).transpose(-1, -2)   # world -> camera
        P = q.new_zeros((B, 7, 7))
        P[:, 0:3, 0:3] = M
        P[:, 3:6, 3:6] = M
        P[:, 6, 6] = 1.0
        T = T @ P
    return T


def tangent_information(gram: torch.Tensor, orientation: torch.Tensor, inv_scale: torch.Tensor,
                        camera_orientations: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,7,7) float64: ``T^T H8 T`` of ``gram[:, :8, :8]`` with ``tangent_map``'s T -- the information about
    (position, rotation vector, log-scale).  In the world frame (``camera_orientations``) the views of one object add."""
    H8 = gram.to(torch.float64).reshape(-1, GRAM_SIZE, GRAM_SIZE)[:, :8, :8]
    T = tangent_map(orientation, inv_scale, camera_orientations).to(H8.device)
    H7 = T.transpose(-1, -2) @ H8 @ T
    return 0.5 * (H7 + H7.transpose(-1, -2))


@dataclass
class PoseUncertainty:
    """What ``pose_covariance`` returns, batched over K objects (float64 but ``rank``).

    information (K,7,7); covariance (K,7,7) = sigma2 * pseudo-inverse over the retained eigen-space; sigma2 (K,) the
    residual variance (NaN where the pixels do not outnumber the rank); rank (K,) int64; position_std (K,3) metres,
    rotation_std_deg (K,3) degrees about the frame's axes, scale_rel_std (K,) -- square roots of the covariance's
    diagonal, within the retained space; unobserved (K,7,7): row i is the eigenvector of the i-th smallest eigenvalue
    if that direction was discarded, zeros otherwise (rows 0 .. 6 - rank are the unobserved directions)."""
    information: torch.Tensor
    covariance: torch.Tensor
    sigma2: torch.Tensor
    rank: torch.Tensor
    position_std: torch.Tensor
    rotation_std_deg: torch.Tensor
    scale_rel_std: torch.Tensor
    unobserved: torch.Tensor


def pose_covariance(information: torch.Tensor, rss: torch.Tensor, count: torch.Tensor, rcond: float = 1e-6,
                    depth_sigma: Optional[float] = None) -> PoseUncertainty:
    """Covariance of (position, rotation vector, log-scale) from the information (K,7,7), the residual sums of
    squares ``rss`` (K,) and the pixel counts (K,).  Eigenvalues at or below ``rcond`` times the largest are
    discarded: ``rank`` counts the others and the covariance is ``sigma2`` times the pseudo-inverse over them.
    ``sigma2 = rss / (count - rank)`` -- NaN where count <= rank -- or ``depth_sigma ** 2`` when the sensor's noise is
    given.  A degenerate row raises nothing: it shows in ``rank`` and NaN."""
    H = information.to(torch.float64).reshape(-1, 7, 7)
    H = 0.5 * (H + H.transpose(-1, -2))
    rss = rss.to(torch.float64).reshape(-1)
    count = count.to(torch.float64).reshape(-1)
    finite = torch.isfinite(H).all(-1).all(-1)
    w, V = torch.linalg.eigh(torch.where(finite[:, None, None], H, torch.zeros_like(H)))   # ascending
    top = w.max(dim=-1).values.clamp(min=0.0)
    keep = (w > rcond * top[:, None]) & (top[:, None] > 0.0) & finite[:, None]
    rank = keep.sum(-1)
    inv = torch.where(keep, 1.0 / torch.where(keep, w, torch.ones_like(w)), torch.zeros_like(w))
    pinv = (V * inv[:, None, :]) @ V.transpose(-1, -2)
    pinv = 0.5 * (pinv + pinv.transpose(-1, -2))
    if depth_sigma is None:
        dof = count - rank
        sigma2 = torch.where(dof > 0, rss / dof.clamp(min=1.0), torch.full_like(rss, float("nan")))
    else:
        sigma2 = torch.full_like(rss, float(depth_sigma) ** 2)
    cov = sigma2[:, None, None] * pinv
    std = torch.sqrt(torch.diagonal(cov, dim1=-2, dim2=-1).clamp(min=0.0))
    unobserved = torch.where(keep[:, :, None], torch.zeros_like(V), V.transpose(-1, -2))
    return PoseUncertainty(information=H, covariance=cov, sigma2=sigma2, rank=rank, position_std=std[:, 0:3],
                           rotation_std_deg=std[:, 3:6] * (180.0 / math.pi), scale_rel_std=std[:, 6],
                           unobserved=unobserved)
