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

Shape.  The loop optimises the latent together with the pose and the two trade against each other, so a pose
covariance conditioned on the decoded shape is too small.  With the decoder's Jacobian (``SDFDecoder.jvp``) the same
call forms the JOINT Gram matrix over pose and T latent directions (``sdfr_render_information_shape``);
``joint_tangent_information`` and ``shape_pose_covariance`` give the (7 + T) x (7 + T) information and covariance, the
pose covariance marginalised over the latent beside the conditional one, and ``sdf_std`` pushes the latent's covariance
back through the Jacobian to a per-voxel standard deviation of the surface.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from .differentiable_renderer import Camera, _check_inputs, _ptr, _stream, _workspace

GRAM_SIZE = 10   # (d0 .. d7, r, 1)


def _sdf_layout(sdf: torch.Tensor, B: int):
    """(R, sdf_view_stride) of an ``sdf`` (R,R,R) shared by B views or (B,R,R,R)"""
    R = sdf.shape[-1]
    if sdf.dim() == 3:
        stride = 0
    elif sdf.dim() == 4 and sdf.shape[0] == B:
        stride = R * R * R
    else:
        raise RuntimeError("sdf must be (R,R,R) or (B,R,R,R)")
    if tuple(sdf.shape[-3:]) != (R, R, R):
        raise RuntimeError("sdf must be cubic")
    return R, stride


def _jacobian_layout(jacobian: torch.Tensor, tangents: Optional[int], B: int, R: int):
    """(Tp, T, jac_view_stride) of a ``jacobian`` (R^3, Tp) shared by B views or (B, R^3, Tp), T = ``tangents`` or Tp"""
    _check_inputs((jacobian, "jacobian"))
    Tp = jacobian.shape[-1]
    T = Tp if tangents is None else int(tangents)
    if jacobian.dim() == 2 and jacobian.shape[0] == R ** 3:
        jstride = 0
    elif jacobian.dim() == 3 and tuple(jacobian.shape[:2]) == (B, R ** 3):
        jstride = R ** 3 * Tp
    else:
        raise RuntimeError("jacobian must be (R^3, Tp) or (B, R^3, Tp)")
    return Tp, T, jstride


def render_information(depth: torch.Tensor, target: torch.Tensor, sdf: torch.Tensor, position: torch.Tensor,
                       orientation: torch.Tensor, inv_scale: torch.Tensor, camera: Camera,
                       inlier_threshold: float = 0.0, workspace: Optional[torch.Tensor] = None,
                       jacobian: Optional[torch.Tensor] = None, tangents: Optional[int] = None) -> torch.Tensor:
    """(B,10,10) float64: per view the Gram matrix of f = (d depth / d (px,py,pz,qx,qy,qz,qw,inv_scale), depth - target, 1)
    over the pixels with depth > 0, target > 0 and -- for ``inlier_threshold`` > 0 -- |target - depth| / target below it.

    ``depth`` is the rendered estimate at the given pose ((H,W) or (B,H,W)), ``target`` the observation; the pose has
    the shapes ``render_depth_gpu`` / ``render_depth_batch`` take: position (3,) or (B,3), orientation (4,) or (B,4),
    inv_scale () or (B,); ``sdf`` (R,R,R) shared by the views or (B,R,R,R).  ``[:8,:8]`` is J^T J, ``[:8,8]`` J^T r,
    ``[8,8]`` sum r^2, ``[9,9]`` the pixel count.  Exactly symmetric, the same bits on every call.

    ``jacobian``: the decoder's Jacobian in ``SDFDecoder.jvp``'s voxel-major layout, (R^3, Tp) shared by the views or
    (B, R^3, Tp), with ``tangents`` = T of its Tp columns in use (default: all).  The result is then (B, 10+T, 10+T), the
    Gram matrix of f = (d0 .. d7, s0 .. s_{T-1}, r, 1) with s_t = d depth / d (latent direction t) over the same pixels
    (``sdfr_render_information_shape``): ``[:8,:8]`` the pose block, ``[8:8+T,8:8+T]`` the latent block, ``[:8+T,8+T]``
    J^T r, ``[8+T,8+T]`` sum r^2, ``[9+T,9+T]`` the count.  1 <= T <= SDFR_INFO_MAX_TANGENTS."""
    _check_inputs((depth, "depth"), (target, "target"), (sdf, "sdf"), (position, "position"),
                  (orientation, "orientation"), (inv_scale, "inv_scale"))
    pos, quat, isc = position.reshape(-1, 3), orientation.reshape(-1, 4), inv_scale.reshape(-1)
    B = pos.shape[0]
    if quat.shape[0] != B or isc.shape[0] != B:
        raise RuntimeError("expected position (B,3), orientation (B,4), inv_scale (B,)")
    H, W = camera.height, camera.width
    if depth.numel() != B * H * W or target.numel() != B * H * W or tuple(depth.shape[-2:]) != (H, W):
        raise RuntimeError(f"expected depth and target of {B} x {H} x {W} pixels")
    R, stride = _sdf_layout(sdf, B)
    fx, fy, cx, cy, _ = camera.get_pinhole_camera_parameters(0.5)
    dev = sdf.device
    L = _lib.lib()
    if jacobian is not None:
        Tp, T, jstride = _jacobian_layout(jacobian, tangents, B, R)
        nbytes = L.sdfr_render_information_shape_workspace_bytes(B, W, H, T)
        if workspace is None and nbytes:
            workspace = _workspace(dev, nbytes)
        ws = _lib.workspace(nbytes, "sdfr_render_information_shape_workspace_bytes", dev, workspace)
        gram = torch.empty((B, GRAM_SIZE + T, GRAM_SIZE + T), dtype=torch.float64, device=dev)
        rc = L.sdfr_render_information_shape(_ptr(depth), _ptr(target), _ptr(sdf), R, stride, _ptr(jacobian), Tp, T,
                                             jstride, _ptr(pos), _ptr(quat), _ptr(isc), B, W, H, cx, cy, fx, fy,
                                             float(inlier_threshold), _ptr(gram), _ptr(ws), ws.numel(), dev.index,
                                             _stream(dev))
        _lib.check(rc, "sdfr_render_information_shape")
        return gram
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


def pc_information(points: torch.Tensor, offsets: Optional[torch.Tensor], sdf: torch.Tensor, position: torch.Tensor,
                   orientation: torch.Tensor, scale: torch.Tensor, jacobian: Optional[torch.Tensor] = None,
                   tangents: Optional[int] = None, max_view_points: Optional[int] = None,
                   workspace: Optional[torch.Tensor] = None, return_inside: bool = False):
    """(B,F,F) float64, F = 10 + T: per view the Gram matrix of f = (d r / d (px,py,pz,qx,qy,qz,qw,inv_scale),
    s0 .. s_{T-1}, r, 1) over ALL points of the view, r the point-cloud residual -- the posed SDF at the observed point,
    what ``pc_loss`` returns; 0 and no gradient outside the volume -- (``sdfr_pc_information``).

    ``points`` (N,3) float32 packed view after view, ``offsets`` (B+1,) int32 (view v owns [offsets[v], offsets[v+1]));
    None: one view of all N points); the pose has ``render_information``'s shapes, with ``scale`` () or (B,) where that
    takes inv_scale -- the derivative's coordinate is inv_scale all the same, so ``tangent_information`` /
    ``joint_tangent_information`` apply to the result as they are; ``sdf`` (R,R,R) shared or (B,R,R,R); ``jacobian`` /
    ``tangents`` as ``render_information`` (T = 0 without).  ``max_view_points``: an upper bound of every view's count
    that the caller knows without reading ``offsets`` back (default: N).  ``[:8+T,:8+T]`` is J^T J, ``[:8+T,8+T]`` J^T r,
    ``[8+T,8+T]`` sum r^2, ``[9+T,9+T]`` the view's point count.  Exactly symmetric, the same bits on every call, a view
    does not depend on its batch.  ``return_inside``: also the (B,) int32 counts of the points inside the volume."""
    _check_inputs((points, "points"), (sdf, "sdf"), (position, "position"), (orientation, "orientation"),
                  (scale, "scale"))
    pos, quat, sc = position.reshape(-1, 3), orientation.reshape(-1, 4), scale.reshape(-1)
    B = pos.shape[0]
    if quat.shape[0] != B or sc.shape[0] != B:
        raise RuntimeError("expected position (B,3), orientation (B,4), scale (B,)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("points must be (N,3)")
    N = points.shape[0]
    if offsets is None:
        if B != 1:
            raise RuntimeError("offsets may be None only for a single view")
    elif not (offsets.is_cuda and offsets.is_contiguous() and offsets.dtype is torch.int32 and tuple(offsets.shape) == (B + 1,)):
        raise RuntimeError(f"offsets must be a contiguous int32 CUDA tensor of shape ({B + 1},)")
    M = N if max_view_points is None else int(max_view_points)
    if offsets is None and M != N:
        raise RuntimeError("without offsets max_view_points is the number of points")
    R, stride = _sdf_layout(sdf, B)
    Tp = T = jstride = 0
    if jacobian is not None:
        Tp, T, jstride = _jacobian_layout(jacobian, tangents, B, R)
        if T < 1:
            raise RuntimeError("tangents must be >= 1 with a jacobian")
    dev = sdf.device
    L = _lib.lib()
    ws = None
    if B > 0 and M > 0:
        nbytes = L.sdfr_pc_information_workspace_bytes(B, M, T)
        if workspace is None and nbytes:
            workspace = _workspace(dev, nbytes)
        ws = _lib.workspace(nbytes, "sdfr_pc_information_workspace_bytes", dev, workspace)
    gram = torch.empty((B, GRAM_SIZE + T, GRAM_SIZE + T), dtype=torch.float64, device=dev)
    inside = torch.empty(B, dtype=torch.int32, device=dev) if return_inside else None
    rc = L.sdfr_pc_information(_ptr(points), _ptr(offsets), B, M, _ptr(pos), _ptr(quat), _ptr(sc), _ptr(sdf), R, stride,
                               _ptr(jacobian), Tp, T, jstride, _ptr(gram), _ptr(inside), _ptr(ws),
                               0 if ws is None else ws.numel(), dev.index, _stream(dev))
    _lib.check(rc, "sdfr_pc_information")
    return (gram, inside) if return_inside else gram


def combine_information(gram_depth: torch.Tensor, gram_pc: torch.Tensor, views: int, pc_weight: float,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(K V, F, F) float64: the Gram matrices of the combined objective
    ``sum rss_d / sum cnt_d + pc_weight sum rss_p / sum M`` of K objects with ``views`` views each, object-major, in the
    form ``lm_step`` takes (``sdfr_information_combine``): per object ``gram_depth + alpha gram_pc`` with
    ``alpha = pc_weight cnt_d / M`` (0 where either count is 0) on all but the last row and column, which stay
    ``gram_depth``'s -- the count is the depth term's.  ``out`` may be ``gram_depth`` (in place); default: a new tensor."""
    V = int(views)
    F = gram_depth.shape[-1]
    if out is None:
        out = torch.empty_like(gram_depth)
    for t, name in ((gram_depth, "gram_depth"), (gram_pc, "gram_pc"), (out, "out")):
        if not (t.is_cuda and t.is_contiguous() and t.dtype is torch.float64 and t.dim() == 3
                and tuple(t.shape) == tuple(gram_depth.shape) and t.shape[-2] == F):
            raise RuntimeError(f"{name} must be a contiguous float64 CUDA tensor of shape (K V, F, F), got "
                               f"{t.dtype} {tuple(t.shape)}")
    if V < 1 or gram_depth.shape[0] % V:
        raise RuntimeError(f"{gram_depth.shape[0]} matrices are not K objects of {V} views")
    dev = gram_depth.device
    rc = _lib.lib().sdfr_information_combine(_ptr(gram_depth), _ptr(gram_pc), gram_depth.shape[0] // V, V,
                                             F - GRAM_SIZE, float(pc_weight), _ptr(out), dev.index, _stream(dev))
    _lib.check(rc, "sdfr_information_combine")
    return out


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


def joint_tangent_information(gram: torch.Tensor, orientation: torch.Tensor, inv_scale: torch.Tensor,
                              camera_orientations: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,7+T,7+T) float64 from the joint Gram matrices (B,10+T,10+T) of ``render_information(jacobian=)``:
    ``tangent_map``'s T on the pose block, the identity on the latent block (the latent is the same vector in every
    frame).  In the world frame (``camera_orientations``) the views of one object add."""
    F = gram.shape[-1]
    L = F - GRAM_SIZE
    if gram.shape[-2] != F or L < 1:
        raise RuntimeError("gram must be (B, 10+T, 10+T) with T >= 1")
    G = gram.to(torch.float64).reshape(-1, F, F)[:, :8 + L, :8 + L]
    T8 = tangent_map(orientation, inv_scale, camera_orientations).to(G.device)
    M = G.new_zeros((G.shape[0], 8 + L, 7 + L))
    M[:, :8, :7] = T8
    M[:, 8:, 7:] = torch.eye(L, dtype=torch.float64, device=G.device)
    Hj = M.transpose(-1, -2) @ G @ M
    return 0.5 * (Hj + Hj.transpose(-1, -2))


@dataclass
class ShapePoseUncertainty:
    """What ``shape_pose_covariance`` returns, batched over K objects; n = 7 + T (float64 but ``rank``).

    information (K,n,n): J^T J / sigma2 with the latent prior added; covariance (K,n,n) its pseudo-inverse over the
    retained space -- [:7,:7] is the pose covariance MARGINALISED over the latent, [7:,7:] the latent's;
    position_std (K,3), rotation_std_deg (K,3), scale_rel_std (K,) from that marginal block;
    conditional: the ``PoseUncertainty`` of the pose block alone, the shape held fixed -- what
    ``SDFPipeline.pose_uncertainty`` reports (its stds are never above the marginal ones in a full-rank problem);
    latent_std (K,T); sigma2 (K,); rank (K,) int64 of ``information``; unobserved (K,n,n): row i is the direction of the
    i-th smallest eigenvalue if it was discarded, zeros otherwise; sdf_std: (K,D,D,D) float32 where it was asked for
    (``SDFPipeline.shape_uncertainty(sdf_std=True)``), else None."""
    information: torch.Tensor
    covariance: torch.Tensor
    pose_covariance: torch.Tensor
    position_std: torch.Tensor
    rotation_std_deg: torch.Tensor
    scale_rel_std: torch.Tensor
    conditional: PoseUncertainty
    latent_std: torch.Tensor
    sigma2: torch.Tensor
    rank: torch.Tensor
    unobserved: torch.Tensor
    sdf_std: Optional[torch.Tensor] = None


def _retained(H: torch.Tensor, rcond: float):
    """eigen-decomposition of the symmetric (K,n,n) H and the mask of the eigenvalues above rcond x the largest (a row
    that is not finite keeps none): ``pose_covariance``'s rule"""
    finite = torch.isfinite(H).all(-1).all(-1)
    w, V = torch.linalg.eigh(torch.where(finite[:, None, None], H, torch.zeros_like(H)))
    top = w.max(dim=-1).values.clamp(min=0.0)
    keep = (w > rcond * top[:, None]) & (top[:, None] > 0.0) & finite[:, None]
    return w, V, keep, finite


def shape_pose_covariance(information: torch.Tensor, rss: torch.Tensor, count: torch.Tensor, latent_prior: float = 1.0,
                          rcond: float = 1e-6, depth_sigma: Optional[float] = None) -> ShapePoseUncertainty:
    """Joint covariance of (position, rotation vector, log-scale, latent) from ``joint_tangent_information``'s J^T J
    (K,7+T,7+T), the residual sums of squares (K,) and the pixel counts (K,).

    ``sigma2`` is formed as in ``pose_covariance`` -- ``rss / (count - rank of J^T J)``, NaN where the pixels do not
    outnumber the rank, or ``depth_sigma ** 2`` -- BEFORE the prior is added.  ``latent_prior`` = lambda adds the VAE's
    N(0, I / lambda) prior as ``lambda I`` on the latent block of ``J^T J / sigma2`` (0: no prior).
    The latent's units are arbitrary beside metres and radians, so before the eigenvalues are compared with ``rcond``
    every latent coordinate is scaled so that its diagonal entry equals the pose block's largest eigenvalue (the pose
    block is not touched, a latent coordinate with a zero diagonal neither); the covariance is mapped back.  A degenerate row raises
    nothing: it shows in ``rank`` and NaN."""
    H = information.to(torch.float64)
    n = H.shape[-1]
    T = n - 7
    if H.shape[-2] != n or T < 1:
        raise RuntimeError("information must be (K, 7+T, 7+T) with T >= 1")
    H = H.reshape(-1, n, n)
    H = 0.5 * (H + H.transpose(-1, -2))
    K = H.shape[0]
    rss = rss.to(torch.float64).reshape(-1)
    count = count.to(torch.float64).reshape(-1)
    conditional = pose_covariance(H[:, :7, :7], rss, count, rcond=rcond, depth_sigma=depth_sigma)
    _, _, keep0, _ = _retained(H, rcond)
    if depth_sigma is None:
        dof = count - keep0.sum(-1)
        sigma2 = torch.where(dof > 0, rss / dof.clamp(min=1.0), torch.full_like(rss, float("nan")))
    else:
        sigma2 = torch.full_like(rss, float(depth_sigma) ** 2)
    prior = H.new_zeros(n)
    prior[7:] = float(latent_prior)
    A = H / sigma2[:, None, None] + torch.diag(prior)
    ok = torch.isfinite(A).all(-1).all(-1)
    A0 = torch.where(ok[:, None, None], A, torch.zeros_like(A))
    tp = torch.linalg.eigvalsh(A0[:, :7, :7])[:, -1].clamp(min=0.0)
    dz = torch.diagonal(A0[:, 7:, 7:], dim1=-2, dim2=-1)
    usable = (dz > 0) & (tp[:, None] > 0)
    c = torch.where(usable, torch.sqrt(tp[:, None] / torch.where(usable, dz, torch.ones_like(dz))), torch.ones_like(dz))
    S = torch.cat([H.new_ones((K, 7)), c], dim=1)
    w, V, keep, _ = _retained(S[:, :, None] * A0 * S[:, None, :], rcond)
    keep = keep & ok[:, None]
    inv = torch.where(keep, 1.0 / torch.where(keep, w, torch.ones_like(w)), torch.zeros_like(w))
    cov = S[:, :, None] * ((V * inv[:, None, :]) @ V.transpose(-1, -2)) * S[:, None, :]
    cov = 0.5 * (cov + cov.transpose(-1, -2))
    cov = torch.where(ok[:, None, None], cov, torch.full_like(cov, float("nan")))
    std = torch.sqrt(torch.diagonal(cov, dim1=-2, dim2=-1).clamp(min=0.0))
    # a discarded eigenvector v of S A S is the direction S v of A
    U = V.transpose(-1, -2) * S[:, None, :]
    U = U / torch.linalg.norm(U, dim=-1, keepdim=True).clamp(min=1e-300)
    unobserved = torch.where(keep[:, :, None], torch.zeros_like(U), U)
    return ShapePoseUncertainty(information=A, covariance=cov, pose_covariance=cov[:, :7, :7], position_std=std[:, 0:3],
                                rotation_std_deg=std[:, 3:6] * (180.0 / math.pi), scale_rel_std=std[:, 6],
                                conditional=conditional, latent_std=std[:, 7:], sigma2=sigma2, rank=keep.sum(-1),
                                unobserved=unobserved)


def sdf_std(jac: torch.Tensor, latent_covariance: torch.Tensor, tangents: Optional[int] = None) -> torch.Tensor:
    """(K,D,D,D) float32: the standard deviation of every voxel of K decoded volumes under a covariance of their
    latents, ``sqrt(max(0, j^T S j))`` with j the voxel's row of ``SDFDecoder.jvp``'s buffer ``jac`` (K, D^3, Tp) and S
    ``latent_covariance`` (K,T,T) (``sdfr_sdf_std``; T = ``tangents``, default S's size)."""
    _check_inputs((jac, "jac"))
    if jac.dim() != 3:
        raise RuntimeError("jac must be (K, D^3, Tp)")
    K, voxels, Tp = jac.shape
    T = latent_covariance.shape[-1] if tangents is None else int(tangents)
    D = round(voxels ** (1.0 / 3.0))
    cov = latent_covariance.to(device=jac.device, dtype=torch.float64).reshape(-1, T, T).contiguous()
    if D ** 3 != voxels or cov.shape[0] != K:
        raise RuntimeError("expected jac (K, D^3, Tp) and latent_covariance (K, T, T)")
    out = torch.empty((K, D, D, D), dtype=torch.float32, device=jac.device)
    rc = _lib.lib().sdfr_sdf_std(_ptr(jac), K, voxels, Tp, T, _ptr(cov), _ptr(out), jac.device.index, _stream(jac.device))
    _lib.check(rc, "sdfr_sdf_std")
    return out
