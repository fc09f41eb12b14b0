"""Looking at a render and at a run: surface normals, colour-mapped and shaded frames, the frames of a trajectory.

The work happens in ``libsdfr_hip.so`` (``csrc/shade.hip``: ``sdfr_render_normals``, ``sdfr_depth_range``,
``sdfr_shade_frames``); tensors are buffers.  The reference draws one matplotlib figure per image and iteration with a
host synchronisation each (simple_setup.py:870-975); here the frames of a whole trajectory are a handful of launches
made AFTER the loop has finished, from the states it recorded, and nothing is read back before the caller asks.
Frames are raw ``W x H`` RGB8 images, not figures: no axes, no margins.  PIL is needed by the two writers only and is
imported inside them; matplotlib is not needed at all (the viridis table is compiled in, ``csrc/colormap_table.hpp``).
"""
import math
import os
from typing import Dict, Optional, Sequence

import torch

from . import _lib
from .differentiable_renderer import Camera, _check_inputs, _ptr, _stream, render_depth_batch

__all__ = ["render_normals", "depth_range", "shade_frames", "trajectory_depth", "trajectory_frames", "write_frames", "write_animation",
           "canonical_view"]

OUTPUTS = ("depth", "depth_error", "shaded")
MESH_COLOR = (0.2, 0.4, 0.7)    # what the reference's player paints meshes with (play_log.py:126)
# the rotation [[-1,0,0],[0,0,1],[0,1,0]] of simple_setup.py:960-962 (y <-> z, x mirrored: half a turn about (0,1,1)) as
# a scalar-last quaternion
CANONICAL_ORIENTATION = (0.0, math.sqrt(0.5), math.sqrt(0.5), 0.0)


def _grid_args(sdf: torch.Tensor, B: int, views_per_state: int = 1):
    R = sdf.shape[-1]
    if tuple(sdf.shape[-3:]) != (R, R, R):
        raise RuntimeError("sdf must be cubic")
    if sdf.dim() == 3:
        return R, 0
    if sdf.dim() == 4 and sdf.shape[0] * views_per_state == B:
        return R, R * R * R
    raise RuntimeError("sdf must be (R,R,R) or (B / views_per_state,R,R,R)")


def _check_poses(positions, orientations, inv_scales, B: int) -> None:
    if positions.shape != (B, 3) or orientations.shape != (B, 4) or inv_scales.shape != (B,):
        raise RuntimeError("expected positions (B,3), orientations (B,4), inv_scales (B,)")


def render_normals(sdf: torch.Tensor, positions: torch.Tensor, orientations: torch.Tensor, inv_scales: torch.Tensor,
                   threshold: float, camera: Camera, depth: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Unit surface normals in the camera frame (OpenGL), (B,H,W,3) float32: at every pixel with ``depth != 0`` the
    normalised gradient of the trilinear SDF at the pixel's hit point, pointing away from the object; zeros elsewhere.
    sdf (R,R,R) shared or (B,R,R,R); poses as ``render_depth_batch`` takes them; depth (B,H,W): the render of the same
    poses, made with ``render_depth_batch`` when not given.  Not differentiable."""
    with torch.no_grad():
        sdf, positions, orientations, inv_scales = (t.detach().contiguous() for t in
                                                    (sdf, positions, orientations, inv_scales))
        if depth is None:
            depth = render_depth_batch(sdf, positions, orientations, inv_scales, threshold, camera)
        depth = depth.detach().contiguous()
        _check_inputs((sdf, "sdf"), (positions, "positions"), (orientations, "orientations"),
                      (inv_scales, "inv_scales"), (depth, "depth"))
        B = positions.shape[0]
        _check_poses(positions, orientations, inv_scales, B)
        W, H = camera.width, camera.height
        if depth.shape != (B, H, W):
            raise RuntimeError("depth must be (B,H,W) of the camera's size")
        R, stride = _grid_args(sdf, B)
        fx, fy, cx, cy, _ = camera.get_pinhole_camera_parameters(0.5)
        dev = sdf.device
        normals = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
        rc = _lib.lib().sdfr_render_normals(_ptr(depth), _ptr(sdf), R, stride, _ptr(positions), _ptr(orientations),
                                            _ptr(inv_scales), B, W, H, cx, cy, fx, fy, _ptr(normals), dev.index,
                                            _stream(dev))
        _lib.check(rc, "sdfr_render_normals")
    return normals


def depth_range(depth: torch.Tensor, shared: bool = False) -> torch.Tensor:
    """(minimum, maximum) over the finite, non-zero pixels of each image of depth (B,H,W) -> (B,2), or of all of them
    with ``shared`` -> (1,2); (0, 0) where there are none.  Exact, on the device: one launch per image set, and for
    ``shared`` over several images a second one that reduces the per-image rows (a row (0, 0) counts for nothing)."""
    depth = depth.detach()
    if depth.dim() == 2:
        depth = depth[None]
    depth = depth.contiguous()
    _check_inputs((depth, "depth"))
    if depth.dim() != 3:
        raise RuntimeError("depth must be (B,H,W) or (H,W)")
    B, H, W = depth.shape
    dev = depth.device
    L = _lib.lib()
    rows = torch.empty((B, 2), dtype=torch.float32, device=dev)
    _lib.check(L.sdfr_depth_range(_ptr(depth), B, W, H, 0, _ptr(rows), dev.index, _stream(dev)), "sdfr_depth_range")
    if not shared or B == 1:
        return rows
    out = torch.empty((1, 2), dtype=torch.float32, device=dev)
    _lib.check(L.sdfr_depth_range(_ptr(rows), 1, 2 * B, 1, 1, _ptr(out), dev.index, _stream(dev)), "sdfr_depth_range")
    return out


def _rgb_word(color: Sequence[int]) -> int:
    r, g, b = (int(c) for c in color)
    if not all(0 <= c <= 255 for c in (r, g, b)):
        raise ValueError("background must be three integers in [0, 255]")
    return (r << 16) | (g << 8) | b


def shade_frames(depth: torch.Tensor, sdf: Optional[torch.Tensor], positions: Optional[torch.Tensor],
                 orientations: Optional[torch.Tensor], inv_scales: Optional[torch.Tensor], camera: Camera,
                 target: Optional[torch.Tensor] = None, views_per_state: int = 1,
                 value_range: Optional[torch.Tensor] = None, error_max: float = 0.05,
                 light: Sequence[float] = (0, 0, 1), ambient: float = 0.25, color: Sequence[float] = MESH_COLOR,
                 background: Sequence[int] = (255, 255, 255),
                 outputs: Sequence[str] = OUTPUTS) -> Dict[str, torch.Tensor]:
    """RGB8 images of B rendered frames in ONE pass: {name: (B,H,W,3) uint8} for the names in `outputs`.

    depth (B,H,W), frames ordered (state, view) with ``views_per_state`` views per state; sdf (R,R,R) or one grid per
    STATE (B / views_per_state,R,R,R); poses per frame, in the frame's camera.  A pixel with ``depth == 0`` gets
    `background` in every image.  Otherwise
      "depth"        viridis of the depth over `value_range` -- (vmin, vmax) as two numbers or a tensor (2,) / (1,2)
                     for all frames, or a tensor (B,2) per frame (a device tensor is used where it is); None: the shared range of `target` if there is one, else of `depth` (``depth_range``,
                     on the device) -- with matplotlib's binning;
      "depth_error"  needs `target` (views_per_state,H,W): viridis of |depth - target| over [0, error_max], background
                     where the target is 0 (simple_setup.py:939-941);
      "shaded"       needs sdf and the poses: Lambert shading of `color` by the surface normal (``render_normals``) with
                     one directional `light` (camera frame, towards the light) over an `ambient` floor.
    """
    names = tuple(outputs)
    if not names or any(n not in OUTPUTS for n in names):
        raise ValueError(f"outputs must be a non-empty selection of {OUTPUTS}")
    depth = depth.detach().contiguous()
    _check_inputs((depth, "depth"))
    if depth.dim() != 3:
        raise RuntimeError("depth must be (B,H,W)")
    B, H, W = depth.shape
    if (W, H) != (camera.width, camera.height):
        raise RuntimeError("depth must have the camera's size")
    V = int(views_per_state)
    dev = depth.device
    R, stride = 2, 0
    if "shaded" in names:
        if sdf is None or positions is None or orientations is None or inv_scales is None:
            raise ValueError("the shaded image needs sdf, positions, orientations and inv_scales")
        sdf, positions, orientations, inv_scales = (t.detach().contiguous() for t in
                                                    (sdf, positions, orientations, inv_scales))
        _check_inputs((sdf, "sdf"), (positions, "positions"), (orientations, "orientations"),
                      (inv_scales, "inv_scales"))
        _check_poses(positions, orientations, inv_scales, B)
        if V >= 1 and B % V == 0:       # (anything else is the library's to refuse)
            R, stride = _grid_args(sdf, B, V)
        else:
            R = sdf.shape[-1]
    else:
        sdf = positions = orientations = inv_scales = None
    if target is not None:
        target = target.detach()
        target = (target[None] if target.dim() == 2 else target).contiguous()
        _check_inputs((target, "target"))
        if target.shape != (max(V, 1), H, W):
            raise RuntimeError("target must be (views_per_state,H,W)")
    if "depth_error" in names and target is None:
        raise ValueError("the error image needs a target")
    rng, rng_stride = None, 0
    if "depth" in names:
        if value_range is None:
            rng = depth_range(target if target is not None else depth, shared=True)
        else:
            # (vmin, vmax) once -- a pair of numbers, a tensor (2,) or (1,2) -- or one row per frame, (B,2); for B = 1
            # the two mean the same
            rng = torch.as_tensor(value_range, dtype=torch.float32).detach().to(dev).contiguous()
            if tuple(rng.shape) in ((2,), (1, 2)):
                rng_stride = 0
            elif tuple(rng.shape) == (B, 2):
                rng_stride = 2
            else:
                raise RuntimeError(f"value_range must be (vmin, vmax), (1,2) or ({B},2), got {tuple(rng.shape)}")
    fx, fy, cx, cy, _ = camera.get_pinhole_camera_parameters(0.5)
    out = {n: torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) for n in names}
    lx, ly, lz = (float(c) for c in light)
    cr, cg, cb = (float(c) for c in color)
    rc = _lib.lib().sdfr_shade_frames(
        _ptr(depth), _ptr(sdf), R, stride, _ptr(positions), _ptr(orientations), _ptr(inv_scales), B, W, H, cx, cy, fx,
        fy, V, _ptr(target) if "depth_error" in names else None, _ptr(rng), rng_stride, float(error_max), lx, ly, lz,
        float(ambient), cr, cg, cb, _rgb_word(background), _ptr(out.get("depth")), _ptr(out.get("depth_error")),
        _ptr(out.get("shaded")), dev.index, _stream(dev))
    _lib.check(rc, "sdfr_shade_frames")
    return out


def canonical_view(camera: Camera, n: int, device) -> tuple:
    """(positions (n,3), orientations (n,4), inv_scales (n,)) of the fixed viewpoint of the ``sdf`` stream: the object
    at the origin of its own frame, turned by the rotation of simple_setup.py:960-962, inv_scale 1, on the optical axis
    at the distance where the bounding sphere of its unit cube (radius sqrt 3) fits the smaller field of view."""
    fx, fy, _, _, _ = camera.get_pinhole_camera_parameters(0.5)
    half = min(math.atan(0.5 * camera.width / abs(fx)), math.atan(0.5 * camera.height / abs(fy)))
    distance = math.sqrt(3.0) / math.sin(half)
    pos = torch.tensor([0.0, 0.0, -distance], dtype=torch.float32, device=device).repeat(n, 1)
    quat = torch.tensor(CANONICAL_ORIENTATION, dtype=torch.float32, device=device).repeat(n, 1)
    return pos, quat, torch.ones(n, dtype=torch.float32, device=device)


def _stack_states(states) -> tuple:
    """a history (list of per-iteration dicts of a loop) or its four stacked tensors -> positions (T,3), orientations
    (T,4), scales (T,), latents (T,L)"""
    if isinstance(states, (list,)) and states and isinstance(states[0], dict):
        return (torch.cat([s["position"].reshape(1, 3) for s in states]),
                torch.cat([s["orientation"].reshape(1, 4) for s in states]),
                torch.cat([s["scale"].reshape(1) for s in states]),
                torch.cat([s["latent"].reshape(1, -1) for s in states]))
    positions, orientations, scales, latents = states
    return positions.reshape(-1, 3), orientations.reshape(-1, 4), scales.reshape(-1), latents.reshape(scales.numel(), -1)


def trajectory_depth(pipeline, states, camera_positions: Optional[torch.Tensor],
                     camera_orientations: Optional[torch.Tensor], view: int = 0) -> tuple:
    """(sdf (T,R,R,R), depth (T,H,W)): the T states of a run decoded in ONE batch and rendered into camera `view` in
    ONE ``render_depth_batch`` -- the world-frame estimate taken into the camera as the loop does it
    (pipeline.py: position_c = q_w2c (position - camera position), orientation_c = q_w2c orientation).  states and
    cameras as ``trajectory_frames`` takes them."""
    with torch.no_grad():
        from .pipeline import quaternion_apply, quaternion_invert, quaternion_multiply
        positions, orientations, scales, latents = (t.detach().to(torch.float32) for t in _stack_states(states))
        T = positions.shape[0]
        sdf = pipeline.vae.decode(latents)[:, 0].contiguous()
        if camera_positions is not None or camera_orientations is not None:
            cam_p = (positions.new_zeros(3) if camera_positions is None
                     else camera_positions.reshape(-1, 3)[view].to(positions))
            cam_q = (positions.new_tensor([0.0, 0.0, 0.0, 1.0]) if camera_orientations is None
                     else camera_orientations.reshape(-1, 4)[view].to(positions))
            q_w2c = quaternion_invert(cam_q)
            positions = quaternion_apply(q_w2c, positions - cam_p)
            orientations = quaternion_multiply(q_w2c.expand(T, 4), orientations)
        depth = render_depth_batch(sdf, positions.contiguous(), orientations.contiguous(), (1.0 / scales).contiguous(),
                                   pipeline.config["threshold"], pipeline.cam)
    return sdf, depth


def trajectory_frames(pipeline, states, depth_images: torch.Tensor, camera_positions: Optional[torch.Tensor],
                      camera_orientations: Optional[torch.Tensor], view: int = 0) -> Dict[str, torch.Tensor]:
    """The frames of a run: {"depth", "depth_error", "sdf"}, each (T,H,W,3) uint8 on the device.

    states: a loop's ``history`` or its four stacked tensors (positions (T,3), orientations (T,4), scales (T,), latents
    (T,L)), world frame; depth_images (N,H,W): the preprocessed observation; cameras (N,3) / (N,4) or None (the origin,
    the identity); view: whose camera and image the first two streams use.
      depth        the estimate rendered into camera `view`, viridis over the range of that view's observation
      depth_error  its absolute difference to the observation over [0, 0.05], background where either has no depth
      sdf          the decoded shape alone, Lambert-shaded, from the fixed viewpoint of ``canonical_view``
    ONE batched decode of the T latents, ONE ``render_depth_batch`` of the T states (``trajectory_depth``), one more from
    the fixed viewpoint, then two ``sdfr_shade_frames`` calls (and the range of the observation): no Python loop over
    states and no host synchronisation -- the result is device tensors."""
    with torch.no_grad():
        cam = pipeline.cam
        if depth_images.dim() == 2:
            depth_images = depth_images[None]
        sdf, depth = trajectory_depth(pipeline, states, camera_positions, camera_orientations, view)
        T, dev = depth.shape[0], depth.device
        target = depth_images[view:view + 1].to(device=dev, dtype=torch.float32).contiguous()
        seen = shade_frames(depth, None, None, None, None, cam, target=target, outputs=("depth", "depth_error"))
        c_pos, c_quat, c_isc = canonical_view(cam, T, dev)
        c_depth = render_depth_batch(sdf, c_pos, c_quat, c_isc, pipeline.config["threshold"], cam)
        shape = shade_frames(c_depth, sdf, c_pos, c_quat, c_isc, cam, views_per_state=1, outputs=("shaded",))
    return {"depth": seen["depth"], "depth_error": seen["depth_error"], "sdf": shape["shaded"]}


def _host_frames(frames):
    if isinstance(frames, torch.Tensor):
        frames = frames.detach().cpu().numpy()
    if frames.ndim == 3:
        frames = frames[None]
    if frames.ndim != 4 or frames.shape[-1] != 3 or frames.dtype.name != "uint8":
        raise ValueError("frames must be (T,H,W,3) uint8")
    return frames


def write_frames(folder: str, frames, first: int = 1) -> list:
    """frames (T,H,W,3) uint8 -> ``folder/{i:06}.png`` for i = first .. first + T - 1 (the reference numbers its frames
    by iteration, from 1: simple_setup.py:925); returns the paths.  Needs PIL."""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    paths = []
    for i, frame in enumerate(_host_frames(frames), start=first):
        paths.append(os.path.join(folder, f"{i:06}.png"))
        Image.fromarray(frame).save(paths[-1])
    return paths


def write_animation(path: str, frames, fps: int = 30) -> str:
    """frames (T,H,W,3) uint8 -> an animated GIF at `path` (looping, `fps` frames per second).  The reference makes an
    mp4 through ffmpeg (simple_setup.py:967-975), which is not a dependency here; a GIF needs PIL alone, at the price of
    a 256-colour palette per frame."""
    from PIL import Image
    images = [Image.fromarray(f) for f in _host_frames(frames)]
    images[0].save(path, format="GIF", save_all=True, append_images=images[1:], duration=max(int(round(1000.0 / fps)), 1),
                   loop=0)
    return path
