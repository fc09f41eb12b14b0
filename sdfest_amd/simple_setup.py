"""``SDFPipeline``: the front door of the render-and-compare estimator, with the call signature of
``sdfest/estimation/simple_setup.py::SDFPipeline`` (:35-89 constructor, :213-226 ``__call__``, :583-596 result).

A caller of the reference replaces ``from sdfest.estimation.simple_setup import SDFPipeline`` by
``from sdfest_amd import SDFPipeline`` and keeps its code: same config dictionary
(``estimation/configs/default.yaml`` + a model file such as ``configs/models/mug.yaml``), same arguments, same
4-tuple back.  Inside, one call is

    _preprocess_depth   one in-place kernel (``sdfr_preprocess_depth``; :671-693)
    _nn_init            the initialisation network's forward (``init_network.nn_init``; :718-844)
    the 50 iterations   the graph-captured loop (``FusedRenderAndCompare``), built and captured on the FIRST call
                        for a number of views and re-bound to every later observation (``rebind``): no allocation,
                        no capture, no Python per iteration (:408-470)
    result selection    :583-596

After the estimate, ``generate_mesh`` turns a latent and a scale into a mesh as the reference's does (:621-669), with
marching cubes on the GPU (``mesh.extract_mesh``) instead of skimage + open3d; ``generate_meshes`` does the same for
the K rows of ``estimate_objects`` in one batched decode and one launch sequence.

What is NOT here (out of scope): plots (``visualize``) and weight downloads -- weights come as state
dicts or from a local file.  Step logs (``log_path``) and animations (``animation_path``) are OPT-IN, with the config key
``step_log: true``: the loop then records its per-iteration states on the device, and what the reference draws
iteration by iteration with a host synchronisation each is made AFTER the loop from those states (``visualization.py``:
the reference's log pickle, raw ``W x H`` frames instead of matplotlib figures, GIFs instead of mp4).  Without the key
the three arguments are accepted and ignored with a warning, as before, and no launch is added.  ``generate_mesh`` returns ``mesh.Mesh`` (device tensors, OBJ / PLY
writers), not an open3d ``TriangleMesh``.
"""
import os
import pickle
import warnings
from typing import Dict, List, Mapping, Optional, Tuple

import torch

from . import _lib
from ._graphs import BoundedCache
from .boxes import sdf_bounds
from .differentiable_renderer import Camera, parse_sdf_grad_mode, render_depth_gpu
from .mesh import Mesh, extract_mesh
from .init_network import NoDepthError, ResidentInit, SDFPoseNet, adjust_categorical_posterior, nn_init
from .pipeline import (FusedRenderAndCompare, MultiObjectRenderAndCompare, _selection_strategy, preprocess_depth,
                       quaternion_apply, quaternion_invert, quaternion_multiply)
from .vae import SDFDecoder

__all__ = ["SDFPipeline", "NoDepthError"]


def _load_state(source, what: str) -> Mapping:
    """a state dict as given, or ``torch.load`` of a LOCAL file (the reference downloads a missing file from
    ``model_url``, sdfest/utils.py:10-43: there is no network here, and a product should not fetch weights)"""
    if isinstance(source, Mapping):
        return source
    for base in ("", os.path.expanduser("~/.sdfest/model_weights/")):
        path = os.path.expanduser(os.path.join(base, str(source)))
        if os.path.exists(path):
            return torch.load(path, map_location="cpu")
    raise FileNotFoundError(f"{what}: no state dict given and {source!r} is not a local file "
                            "(weights are not downloaded; pass vae_state_dict= / init_state_dict=)")


def _event(device) -> "torch.cuda.Event":
    """a timing event recorded on `device`'s current stream -- the stream the loop launches on"""
    event = torch.cuda.Event(enable_timing=True)
    event.record(torch.cuda.current_stream(device))
    return event


class _TimedHistory(list):
    """a loop's ``history`` that also records an event on the loop's stream behind every entry: the time of every
    iteration without a synchronisation per iteration (read after the loop, ``_StepRecord.timestamps``)"""

    def __init__(self, device):
        super().__init__()
        self.device = device
        self.events = []

    def append(self, entry) -> None:
        super().append(entry)
        self.events.append(_event(self.device))


class _StepRecord:
    """what one ``__call__`` under ``step_log`` keeps: the inputs of the first view as they came, the preprocessed
    observation and the cameras the loop was bound to, the initial estimate, the loop's history and the events that
    time them.  Device tensors; nothing is read back here."""

    def __init__(self, device, start, depth_images, masks, color_images, animation_path):
        self.device = device
        self.start = start           # recorded at the top of the call
        # (the depth is preprocessed in place further on: the animation's depth_input.png needs the first view as given)
        self.raw_depth = None
        if animation_path is not None:
            self.raw_depth = depth_images[0].detach().to(device, torch.float32).clone()
        self.masks = masks.detach()
        self.color = color_images.detach() if isinstance(color_images, torch.Tensor) else color_images
        self.history = _TimedHistory(device)
        self.inputs_done = self.init_done = None     # events behind the preprocessing / behind the initialisation

    def begin(self, loop, position, orientation, scale, latent) -> None:
        """in front of the loop: the observation as the loop holds it, and the estimate it starts from"""
        self.target = loop.target.detach().clone()
        self.cam_pos, self.cam_quat = loop.cam_pos_all.detach().clone(), loop.cam_quat_all.detach().clone()
        self.initial = (position.detach().reshape(1, 3).clone(), orientation.detach().reshape(1, 4).clone(),
                        scale.detach().reshape(1).clone(), latent.detach().reshape(1, -1).clone())
        self.init_done = _event(self.device)

    def states(self) -> tuple:
        keys = ("position", "orientation", "scale", "latent")
        shapes = ((1, 3), (1, 4), (1,), (1, -1))
        return tuple(torch.cat([first] + [h[k].reshape(shape) for h in self.history])
                     for first, k, shape in zip(self.initial, keys, shapes))

    def timestamps(self) -> list:
        """seconds since the call began: [the inputs, the initial estimate, every iteration]; waits for the last event"""
        events = [self.inputs_done, self.init_done] + self.history.events
        events[-1].synchronize()
        return [self.start.elapsed_time(e) * 1e-3 for e in events]


class SDFPipeline:
    """SDF pose and shape estimation pipeline (reference: simple_setup.py:35-89).

    config: the reference's dictionary -- ``device``, ``camera`` {width, height, fx, fy, cx, cy, pixel_center},
    ``threshold``, ``max_iterations``, ``depth_weight``, ``pc_weight``, ``nn_weight``, ``mean_shape``, ``init_view``,
    ``init`` {backbone_type, backbone, head_type, head, normalize_pose, model}, ``vae`` {latent_size, decoder, tsdf,
    model} (or ``init["vae"]``), optionally ``far_field``, ``result_selection_strategy``,
    ``relative_inlier_threshold``, ``orientation_hypotheses`` (N > 1: ``__call__`` refines the N most probable
    orientation cells side by side and returns the best supported one, ``estimate_hypotheses``; not in the reference),
    ``gauss_newton_iterations`` (n > 0: ``__call__``, ``estimate_objects``, ``estimate_frames`` and
    ``estimate_hypotheses`` end with ``refine(n)`` and return the refined estimate; default 0; not in the reference),
    ``gauss_newton_pc_weight`` (the weight of the point-cloud term in ``refine``'s objective; default 0.0: none).
    vae_state_dict / init_state_dict: the state dicts of the reference's ``SDFVAE`` (keys ``decoder.*``; encoder
    keys are ignored) and ``SDFPoseNet``; default: ``torch.load`` of ``config[...]["model"]`` if that file exists.
    init_network: an object called like ``nn_init``'s network, or a callable
    ``(depth_images, camera_positions, camera_orientations, prior, training_prior) -> (latent (1,L), position (1,3),
    scale (1,), orientation (1,4))`` replacing ``_nn_init`` altogether (tests, or a caller with its own initialiser).
    """

    def __init__(self, config: Dict, vae_state_dict: Optional[Mapping] = None,
                 init_state_dict: Optional[Mapping] = None, init_network=None, resident_init: bool = True) -> None:
        self._parse_config(config)
        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise RuntimeError("sdfest_amd runs on the GPU only (config['device'] must be a cuda device)")
        self._dev = torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev
        _selection_strategy(config)     # (the reference raises at the END of a call, :592-596; a typo fails early here)

        self.resolution = 64
        vae_state = _load_state(vae_state_dict if vae_state_dict is not None else self.vae_config.get("model"),
                                "vae")
        self.vae = SDFDecoder.from_config(self.vae_config, vae_state, device=self._dev, sdf_size=self.resolution)

        self._nn_init_override = None
        if callable(init_network) and not isinstance(init_network, SDFPoseNet):
            self._nn_init_override = init_network
            self.init_network = None
        elif init_network is not None:
            self.init_network = init_network
        else:
            if self.init_config["backbone_type"] != "VanillaPointNet" or self.init_config["head_type"] != "SDFPoseHead":
                raise NotImplementedError("the initialisation network is VanillaPointNet + SDFPoseHead "
                                          "(simple_setup.py:27)")
            init_state = _load_state(init_state_dict if init_state_dict is not None
                                     else self.init_config.get("model"), "init")
            self.init_network = SDFPoseNet(self.init_config["backbone"], self.init_config["head"],
                                           self.vae_config["latent_size"], init_state, device=self._dev)

        self.cam = Camera(**self.camera_config)
        # a plain attribute, as in the reference (:84-86; real_data.py:230-243 replaces it at run time)
        self.render = lambda sdf, pos, quat, i_s: render_depth_gpu(
            sdf, pos, quat, i_s, None, None, None, config["threshold"], self.cam, self.sdf_grad_mode)
        self.config = config
        self.log_data = []
        limit = self.MAX_CACHED_LOOPS
        self._loops = BoundedCache(limit)     # (views, shape_optimization) -> the captured loop, re-bound per call
        # resident_init: the initialisation network as a captured launch sequence with nothing read back
        # (init_network.ResidentInit) where its architecture allows; False: the host-driven nn_init (two host reads)
        self._resident_wanted = bool(resident_init)
        self._residents = BoundedCache(limit)
        # estimate_objects: per (K, shape_optimization, V, tracking) / per (K, V)
        self._multi_loops, self._resident_objects = BoundedCache(limit), BoundedCache(limit)
        # estimate_hypotheses: per N / the last call's record
        self._resident_hypotheses, self._last_hypotheses = BoundedCache(limit), None
        self._refiners = BoundedCache(limit)      # refine: per (K, V, shape_optimization, point-cloud term on / off)
        self._ignored_warned = False
        self._trajectory = None                   # step_log: the last call's states and what they were fitted to

    def _parse_config(self, config: Dict) -> None:
        """simple_setup.py:91-109"""
        self.device = config["device"]
        self.init_config = config["init"]
        self.vae_config = config["vae"] if "vae" in config else self.init_config["vae"]
        self.camera_config = config["camera"]
        self.result_selection_strategy = config.get("result_selection_strategy", "last_iteration")
        self._relative_inlier_threshold = config.get("relative_inlier_threshold", 0.03)
        # (the reference sets _far_field only when the key exists and then reads it unconditionally, :106-107, :692:
        # without the key its _preprocess_depth raises AttributeError; None here = no far-field clipping)
        self._far_field = config.get("far_field")
        self.sdf_grad_mode = parse_sdf_grad_mode(config.get("sdf_grad_mode"))
        self.step_log = bool(config.get("step_log", False))
        self.config = config

    # ---- the reference's helpers, same names ------------------------------------------------------------------
    def _preprocess_depth(self, depth_images: torch.Tensor, masks: torch.Tensor) -> None:
        """simple_setup.py:671-693, in place"""
        preprocess_depth(depth_images, masks, self._far_field)

    _adjust_categorical_posterior = staticmethod(adjust_categorical_posterior)    # :977-1009

    def _nn_init(self, depth_images, camera_positions, camera_orientations, prior_orientation_distribution=None,
                 training_orientation_distribution=None) -> Tuple:
        """simple_setup.py:718-844: (latent (1,L), position (1,3), scale (1,), orientation (1,4)), world frame"""
        if self._nn_init_override is not None:
            return self._nn_init_override(depth_images, camera_positions, camera_orientations,
                                          prior_orientation_distribution, training_orientation_distribution)
        return nn_init(self.init_network, self.cam, depth_images, camera_positions, camera_orientations, self.config,
                       normalize_pose=bool(self.init_config.get("normalize_pose", False)),
                       prior_orientation_distribution=prior_orientation_distribution,
                       training_orientation_distribution=training_orientation_distribution)

    def _resident_init(self, views: int):
        """the captured form of ``_nn_init`` for `views` images, or None where only the host-driven form applies"""
        if not self._resident_wanted or self._nn_init_override is not None or not isinstance(self.init_network, SDFPoseNet):
            return None
        return self._residents.get_or_build(views, lambda: self._new_resident(views, self.config))

    def _new_resident(self, views: int, config: Dict, **kwargs):
        """a ``ResidentInit`` of this pipeline's network, or None where its architecture only allows the host-driven form"""
        try:
            return ResidentInit(self.init_network, self.cam, views, config,
                                normalize_pose=bool(self.init_config.get("normalize_pose", False)), **kwargs)
        except NotImplementedError:
            return None

    def generate_depth(self, position, orientation, scale, latent) -> torch.Tensor:
        """simple_setup.py:609-619"""
        sdf = self.vae.decode(latent)
        return self.render(sdf[0, 0], position, orientation, 1 / scale)

    def generate_mesh(self, latent: torch.Tensor, scale: torch.Tensor, complete_mesh: bool = False) -> Optional[Mesh]:
        """simple_setup.py:621-669: the mesh of latent (1,L) at relative scale (1,), without pose; None if the config
        has no ``iso_threshold`` (the reference's ``except KeyError``).  complete_mesh: pad the SDF with 1.0 first (a
        closed mesh).  ValueError if the level lies outside the decoded SDF's range, as skimage raises."""
        with torch.no_grad():
            sdf = self.vae.decode(latent)
            try:
                level = self.config["iso_threshold"]
            except KeyError:
                return None
            mesh = extract_mesh(sdf[0, 0], level, complete=complete_mesh)
        mesh.update_scale(float(scale.reshape(-1)[0]), rel_scale=True)
        return mesh

    def generate_meshes(self, latents: torch.Tensor, scales: torch.Tensor,
                        complete_mesh: bool = False) -> Optional[List[Mesh]]:
        """``generate_mesh`` for K objects at once (the rows of ``estimate_objects``): latents (K,L), scales (K,) ->
        K meshes from one batched decode and one marching-cubes launch sequence.  The reference has none (its
        generate_mesh "only supports batch size 1")."""
        with torch.no_grad():
            sdf = self.vae.decode(latents)
            try:
                level = self.config["iso_threshold"]
            except KeyError:
                return None
            meshes = extract_mesh(sdf[:, 0], level, complete=complete_mesh)
        for m, s in zip(meshes, scales.reshape(-1).tolist()):
            m.update_scale(float(s), rel_scale=True)
        return meshes

    def bounding_boxes(self, position: torch.Tensor, orientation: torch.Tensor, scale: torch.Tensor,
                       latent: torch.Tensor, complete_mesh: bool = True):
        """The oriented bounding boxes of K estimates -- the 4-tuple of ``__call__`` (K = 1) or the rows of
        ``estimate_objects`` / ``estimate_frames``: position (K,3), orientation (K,4), scale (K,), latent (K,L) ->
        (center (K,3), orientation (K,4), extents (K,3)) float64 on the device, the boxes ``generate_meshes(latent, scale,
        complete_mesh)[k]`` posed with row k returns from ``oriented_box()``: center = position + R(q) (scale (lo + hi)
        / 2), extents = scale (hi - lo).  One batched decode and one ``sdfr_sdf_bounds`` call (``boxes.sdf_bounds``):
        no mesh is made.  None if the config has no ``iso_threshold``, as ``generate_mesh``; ``ValueError`` naming the
        row whose decoded SDF the level does not cross (where ``generate_mesh`` raises).  The reference has none."""
        with torch.no_grad():
            sdf = self.vae.decode(latent)
            try:
                level = self.config["iso_threshold"]
            except KeyError:
                return None
            lo, hi, crossed = sdf_bounds(sdf[:, 0], level, complete=complete_mesh)
            empty = torch.nonzero(crossed == 0).flatten().tolist()
            if empty:
                raise ValueError(f"Surface level must be within volume data range (row {empty[0]}: no grid edge of the "
                                 f"decoded SDF crosses the level {level})")
            # float64 from here: the boxes are what box_iou reads, and an fp32 centre would carry the position's rounding
            lo, hi = lo.double(), hi.double()
            s = scale.detach().reshape(-1, 1).to(lo)
            q = orientation.detach().reshape(-1, 4).to(lo)
            unit = q / q.norm(dim=1, keepdim=True)      # as box_iou normalises the quaternion it is given
            center = position.detach().reshape(-1, 3).to(lo) + quaternion_apply(unit, s * ((lo + hi) / 2))
            return center, q, s * (hi - lo)

    # per kind (a caller whose number of views or objects varies from call to call re-builds instead of collecting
    # buffers without bound): a loop holds its point clouds at capacity (3.7 MB per 640x480 view) and its graphs
    MAX_CACHED_LOOPS = 4

    def _loop(self, views: int, shape_optimization: bool) -> FusedRenderAndCompare:
        key = (int(views), bool(shape_optimization))
        return self._loops.get_or_build(key, lambda: FusedRenderAndCompare(
            self.vae, self.cam, self.config, views=views, shape_optimization=shape_optimization, device=self._dev,
            sdf_grad_mode=self.sdf_grad_mode))

    def __call__(self, depth_images: torch.Tensor, masks: torch.Tensor, color_images: torch.Tensor,
                 visualize: bool = False, camera_positions: Optional[torch.Tensor] = None,
                 camera_orientations: Optional[torch.Tensor] = None, log_path: Optional[str] = None,
                 shape_optimization: bool = True, animation_path: Optional[str] = None,
                 point_constraint: Optional[Tuple[torch.Tensor]] = None,
                 prior_orientation_distribution: Optional[torch.Tensor] = None,
                 training_orientation_distribution: Optional[torch.Tensor] = None) -> tuple:
        """Infer pose, size and latent shape from depth and mask -- arguments as simple_setup.py:213-296.

        depth_images (N,H,W) or (H,W): masked and far-field-clipped IN PLACE (pass a copy if the full depth is used
        afterwards); masks: same shape, bool; color_images: unused (visualisation only in the reference).
        Returns (position (1,3), orientation (1,4) normalised scalar-last, scale (1,), latent (1,L)).

        With ``step_log: true`` in the config the loop records its states (the estimate is bit for bit the one without
        the key): ``last_trajectory()`` returns the initial estimate and the ``max_iterations`` iterates,
        ``render_trajectory()`` their frames; log_path: the reference's pickle ``{"config", "log"}`` -- the inputs
        (:339-349), the initial estimate (:363-373), one entry per iteration (:482-490), CPU tensors of the reference's
        shapes, which ``play_log.py`` reads; ``timestamp`` is seconds since the call began, from events recorded on the
        loop's stream between iterations and read after the loop (no synchronisation per iteration).  animation_path:
        the reference's folder (:870-912) -- ``depth/``, ``depth_error/``, ``sdf/`` with ``{iteration:06}.png`` from 1,
        ``color_input.png``, ``depth_input.png``, ``mask.png``, ``preprocessed_depth_input.png`` (the first view; the
        depth ones through the colour map) and ``depth.gif``, ``depth_error.gif``, ``sdf.gif`` (the reference: mp4
        through ffmpeg).  Frames are raw ``W x H`` images, not matplotlib figures.  ``visualize`` stays ignored, and
        the forms without a single trajectory (``orientation_hypotheses > 1``, a loop sharded over ranks) raise
        ``NotImplementedError`` when a path is given."""
        recording = self.step_log
        if recording:
            # seconds since HERE are the log's timestamps; and whatever this call does -- a form that records nothing,
            # an exception -- no earlier call's trajectory is left to be taken for this one's
            start = _event(self._dev)
            self._trajectory = None
        ignored = visualize or (not recording and (log_path is not None or animation_path is not None))
        if ignored and not self._ignored_warned:
            warnings.warn("sdfest_amd.SDFPipeline: visualize / log_path / animation_path are accepted and ignored "
                          "(plots, step logs and animations are outside the hot path)")
            self._ignored_warned = True
        wants_files = recording and (log_path is not None or animation_path is not None)
        n_hypotheses = int(self.config.get("orientation_hypotheses", 1))
        if n_hypotheses != 1 and wants_files:
            raise NotImplementedError("step_log: orientation_hypotheses > 1 refines several estimates side by side and has "
                                      "no single trajectory to log or animate")
        if n_hypotheses != 1:     # (the default path below is untouched by the key's absence or 1)
            if point_constraint is not None:
                raise ValueError("point_constraint cannot be combined with orientation_hypotheses > 1: the K-row loop "
                                 "(MultiObjectRenderAndCompare) has no point constraint")
            return self.estimate_hypotheses(depth_images, masks, color_images, hypotheses=n_hypotheses,
                                            camera_positions=camera_positions, camera_orientations=camera_orientations,
                                            shape_optimization=shape_optimization,
                                            prior_orientation_distribution=prior_orientation_distribution,
                                            training_orientation_distribution=training_orientation_distribution)
        # batch dimension (:306-318)
        if depth_images.dim() == 2:
            depth_images = depth_images.unsqueeze(0)
            masks = masks.unsqueeze(0)
            if camera_positions is not None:
                camera_positions = camera_positions.unsqueeze(0)
            if camera_orientations is not None:
                camera_orientations = camera_orientations.unsqueeze(0)
            if prior_orientation_distribution is not None:
                prior_orientation_distribution = prior_orientation_distribution.unsqueeze(0)
        n_imgs = depth_images.shape[0]
        dev = self._dev
        # (the default cameras -- the origin, the identity: :327-331 -- are left as None for ``rebind``, which writes them
        # into the loop's own buffers; only the host-driven initialisation below needs them as tensors)

        loop = self._loop(n_imgs, shape_optimization)
        if wants_files and loop.group is not None:
            raise NotImplementedError("step_log: a loop sharded over ranks holds a part of the views on every rank and "
                                      "has no single trajectory to log or animate")
        record = _StepRecord(dev, start, depth_images, masks, color_images, animation_path) if recording else None
        with torch.no_grad():
            # :333-334, and the observation into the loop's buffers in the same pass
            if (depth_images.is_cuda and depth_images.dtype is torch.float32 and depth_images.is_contiguous()
                    and depth_images.device == dev):
                loop.rebind(depth_images, camera_positions, camera_orientations, point_constraint, masks=masks,
                            far_field=self._far_field)
            else:
                # any other tensor the reference would take (another dtype or device, a strided view): its own two
                # in-place assignments, then the copy into the loop's buffers
                depth_images[~masks.to(device=depth_images.device, dtype=torch.bool)] = 0
                if self._far_field is not None:
                    depth_images[depth_images > self._far_field] = 0
                loop.rebind(depth_images, camera_positions, camera_orientations, point_constraint)
                depth_images = loop.target if loop.group is None else depth_images.to(dev, torch.float32)
            if record is not None:
                record.inputs_done = _event(dev)
            # :352-359
            resident = self._resident_init(n_imgs)
            if resident is not None:
                # on the loop's own (address-stable) buffers: the preprocessed images and the cameras rebind left there
                latent_shape, position, scale, orientation = resident(
                    loop.target, loop.cam_pos_all, loop.cam_quat_all, prior_orientation_distribution,
                    training_orientation_distribution)
            else:
                latent_shape, position, scale, orientation = self._nn_init(
                    depth_images, loop.cam_pos_all if camera_positions is None else camera_positions,
                    loop.cam_quat_all if camera_orientations is None else camera_orientations,
                    prior_orientation_distribution, training_orientation_distribution)
            # :381-470
            if record is None:
                position, orientation, scale, latent_shape = loop(position, orientation, scale, latent_shape)
            else:
                record.begin(loop, position, orientation, scale, latent_shape)
                position, orientation, scale, latent_shape = loop(position, orientation, scale, latent_shape,
                                                                  history=record.history)
            if resident is not None and resident.empty_views():
                # (:780-781 -- known only now: the counts were never waited for in front of the launches)
                raise NoDepthError
        self._last_loop = loop
        self._last_estimate = loop
        if record is not None:
            self._trajectory = record
            if log_path is not None:
                self._write_log(record, log_path)
            if animation_path is not None:
                self._write_animation(record, animation_path)
        # :583-596 -- "best_inlier_ratio" returns the tensors the reference stored, which its optimiser went on
        # updating in place: the last iterate as well (pipeline._BestEstimate); the snapshot at the best ratio is
        # self.best_estimate()
        return self._gauss_newton((position, orientation, scale, latent_shape))

    # ---- step_log: the last call's trajectory --------------------------------------------------------------------
    def _recorded(self) -> "_StepRecord":
        if self._trajectory is None:
            raise RuntimeError("no trajectory: set step_log: true in the config and call the pipeline first")
        return self._trajectory

    def last_trajectory(self) -> tuple:
        """(positions (T,3), orientations (T,4), scales (T,), latents (T,L)) of the last ``__call__`` under
        ``step_log: true``, T = max_iterations + 1: the initial estimate, then the loop's iterate after every iteration
        (the last row is the loop's result -- what the call returned, before any ``gauss_newton_iterations``).  World
        frame, device tensors."""
        return self._recorded().states()

    def render_trajectory(self, view: int = 0) -> Dict[str, torch.Tensor]:
        """The frames of the last trajectory in camera `view`: ``visualization.trajectory_frames`` -- {"depth",
        "depth_error", "sdf"}, each (T,H,W,3) uint8 on the device, from one batched decode, two batched renders and two
        shading passes."""
        from .visualization import trajectory_frames
        r = self._recorded()
        return trajectory_frames(self, r.states(), r.target, r.cam_pos, r.cam_quat, view=view)

    def _write_log(self, record: "_StepRecord", log_path: str) -> None:
        """the reference's pickle (:339-349, :363-373, :482-490; written as simple_setup.py's ``_write_log_data``)"""
        positions, orientations, scales, latents = (t.cpu() for t in record.states())
        stamps = record.timestamps()
        cams = {"camera_positions": record.cam_pos.cpu(), "camera_orientations": record.cam_quat.cpu()}
        log = [dict({"timestamp": stamps[0], "depth_images": record.target.cpu(),
                     "color_images": record.color.cpu() if isinstance(record.color, torch.Tensor) else record.color,
                     "masks": record.masks.cpu()}, **cams)]
        for t in range(positions.shape[0]):
            entry = {"timestamp": stamps[1 + t]}
            if t == 0:
                entry.update(cams)
            entry.update({"latent_shape": latents[t:t + 1].clone(), "position": positions[t:t + 1].clone(),
                          "scale_inv": 1 / scales[t:t + 1], "orientation": orientations[t:t + 1].clone()})
            log.append(entry)
        with open(log_path, "wb") as f:
            pickle.dump({"config": self.config, "log": log}, f)

    def _write_animation(self, record: "_StepRecord", animation_path: str) -> None:
        from .visualization import depth_range, shade_frames, write_animation, write_frames
        from PIL import Image
        os.makedirs(animation_path, exist_ok=True)
        frames = self.render_trajectory(view=0)
        for name in ("depth", "depth_error", "sdf"):
            host = frames[name][1:].cpu()           # the reference draws after every iteration: 1 .. max_iterations
            write_frames(os.path.join(animation_path, name), host, first=1)
            if host.shape[0]:
                write_animation(os.path.join(animation_path, f"{name}.gif"), host)
        inputs = torch.stack([record.raw_depth, record.target[0]])
        # each image over its own range, as the reference's imshow scales each by itself (a far wall in the raw depth
        # must not squeeze the preprocessed image into a few bins)
        mapped = shade_frames(inputs, None, None, None, None, self.cam, value_range=depth_range(inputs),
                              outputs=("depth",))["depth"]
        Image.fromarray(mapped[0].cpu().numpy()).save(os.path.join(animation_path, "depth_input.png"))
        Image.fromarray(mapped[1].cpu().numpy()).save(os.path.join(animation_path,
                                                                         "preprocessed_depth_input.png"))
        Image.fromarray((record.masks[0].cpu().numpy() != 0).astype("uint8") * 255).save(
            os.path.join(animation_path, "mask.png"))
        color = record.color[0] if isinstance(record.color, torch.Tensor) and record.color.dim() == 4 else record.color
        color = torch.as_tensor(color).detach().cpu()
        if color.is_floating_point():
            color = (color.clamp(0, 1) * 255).round()
        Image.fromarray(color.to(torch.uint8).numpy()).save(os.path.join(animation_path, "color_input.png"))

    def estimate_objects(self, depth_images: torch.Tensor, masks: torch.Tensor,
                         camera_positions: Optional[torch.Tensor] = None,
                         camera_orientations: Optional[torch.Tensor] = None, shape_optimization: bool = True,
                         prior_orientation_distribution: Optional[torch.Tensor] = None,
                         training_orientation_distribution: Optional[torch.Tensor] = None,
                         log_path: Optional[str] = None, animation_path: Optional[str] = None) -> tuple:
        """The K detected objects of ONE frame at once: what a caller of the reference does with a loop of K
        ``pipeline(depth, mask_k, color)`` calls (one per instance mask), as one call whose K estimates are optimised side
        by side (``pipeline.MultiObjectRenderAndCompare``: one launch sequence per iteration for all of them).

        depth_images (H,W): the frame (NOT modified: every object gets its own masked copy); masks (K,H,W) bool: the
        instance masks; camera_positions (3,) / camera_orientations (4,): the camera in the world (default: the origin).
        Or SEVERAL views of the same K objects (two cameras, or one that moved), as ``__call__`` takes them: depth_images
        (V,H,W), masks (K,V,H,W), camera_positions (V,3), camera_orientations (V,4) -- every view needs every object in it.
        The initialisation network sees each object's first view (``init_view: first``, camera 0); ``init_view: best``
        with V > 1 is not implemented.
        prior_orientation_distribution (K,C) / training_orientation_distribution (C,): as in ``__call__``, one row per
        object.  Returns position (K,3), orientation (K,4), scale (K,), latent (K,L) -- row k follows what
        ``pipeline(depth, masks[k], color, camera_positions=..., camera_orientations=...)`` estimates for object k TO
        ROUNDING, tested to 1 % of an Adam step per iteration: the single call runs its render pair as one launch
        (``FusedRenderAndCompare(fused_render=)``: the depth loss's weight / count multiplies sums instead of terms), and with
        shape optimisation a batch of latents takes other, equivalent decoder kernels than a single one (the direct
        convolution from 8 latents on, the tiled resize from 2, no split-K above 16).  Against the single loop in its
        two-launch form the pose-only rows are BIT FOR BIT the same (tests/test_multi_object_gpu.py).
        The rows are the LAST iterate for both values of ``result_selection_strategy``, as ``__call__``'s are; with
        "best_inlier_ratio" every object's inlier bookkeeping (:177-211, on its last view) runs beside the loop and
        ``best_estimates()`` returns it.
        ``NoDepthError`` for an (object, view) without a valid depth pixel is raised AFTER the call's work was
        enqueued (the counts are read behind the launches), where the reference raises before optimising (:780-781).
        log_path / animation_path: K estimates have no single trajectory -- ``NotImplementedError`` under ``step_log``,
        ignored with ``__call__``'s warning without it."""
        self._no_step_files("estimate_objects", log_path, animation_path)
        if depth_images.dim() == 2 and masks.dim() == 3 and tuple(masks.shape[1:]) == tuple(depth_images.shape):
            V = 1
        elif (depth_images.dim() == 3 and masks.dim() == 4 and masks.shape[1] == depth_images.shape[0]
              and tuple(masks.shape[2:]) == tuple(depth_images.shape[1:])):
            V = int(depth_images.shape[0])
        else:
            raise ValueError("depth_images (H,W) and masks (K,H,W), or depth_images (V,H,W) and masks (K,V,H,W), "
                             "are expected")
        if V > 1 and self.config.get("init_view", "first") != "first":
            raise NotImplementedError("estimate_objects with several views initialises from each object's first view "
                                      f"(init_view: first), not init_view: {self.config.get('init_view')}")
        K = int(masks.shape[0])
        loop = self._objects_loop(K, V, shape_optimization)
        with torch.no_grad():
            H, W = loop.H, loop.W
            loop.rebind(depth_images.reshape(V, H, W), camera_positions, camera_orientations,
                        masks=masks.reshape(K, V, H, W), far_field=self._far_field)
            return self._run_objects(loop, prior_orientation_distribution, training_orientation_distribution)

    def _no_step_files(self, what: str, log_path, animation_path) -> None:
        if log_path is None and animation_path is None:
            return
        if self.step_log:
            raise NotImplementedError(f"step_log: {what} refines K estimates side by side and has no single trajectory "
                                      "to log or animate; call the pipeline per object for a log")
        if not self._ignored_warned:
            warnings.warn("sdfest_amd.SDFPipeline: visualize / log_path / animation_path are accepted and ignored "
                          "(plots, step logs and animations are outside the hot path)")
            self._ignored_warned = True

    def _objects_loop(self, K: int, V: int, shape_optimization: bool) -> MultiObjectRenderAndCompare:
        """the K-row loop of ``estimate_objects`` and ``estimate_frames``, built on first use and kept"""
        track = self.result_selection_strategy == "best_inlier_ratio"
        key = (K, bool(shape_optimization), V, track)
        return self._multi_loops.get_or_build(key, lambda: MultiObjectRenderAndCompare(
            self.vae, self.cam, self.config, K, shape_optimization=shape_optimization, device=self._dev,
            sdf_grad_mode=self.sdf_grad_mode, views=V, track_inliers=track))

    def _run_objects(self, loop: MultiObjectRenderAndCompare, prior_orientation_distribution,
                     training_orientation_distribution) -> tuple:
        """initialise the K rows of a bound loop from each row's first view and run it (under ``torch.no_grad``)"""
        K, V, H, W = loop.K, loop.V, loop.H, loop.W
        first = loop.target.view(K, V, H, W)[:, 0]     # every object's first view: K contiguous images
        resident = None
        if self._resident_wanted and self._nn_init_override is None and isinstance(self.init_network, SDFPoseNet):
            # (per (K, V): its captured sequence holds the addresses of K images V images apart)
            resident = self._resident_objects.get_or_build((K, V), lambda: self._new_resident(
                K, dict(self.config, init_view="first"), objects=True))
        if resident is not None:
            latent, position, scale, orientation = resident(first, loop.cam_pos, loop.cam_quat,
                                                            prior_orientation_distribution,
                                                            training_orientation_distribution)
        else:     # the host-driven form, object by object
            rows = []
            for k in range(K):
                prior = prior_orientation_distribution[k:k + 1] if prior_orientation_distribution is not None else None
                rows.append(self._nn_init(first[k:k + 1], loop.cam_pos[0:1], loop.cam_quat[0:1], prior,
                                          training_orientation_distribution))
            latent, position, scale, orientation = (torch.cat([r[i].reshape(1, -1) for r in rows]) for i in range(4))
            scale = scale.reshape(K)
        out = loop(position, orientation, scale, latent)
        self._last_multi_loop = loop
        self._last_estimate = loop
        if resident is not None and resident.empty_views():
            raise NoDepthError
        if V > 1 and bool((loop.counts == 0).any()):     # (the initialisation saw the first views only)
            raise NoDepthError
        return self._gauss_newton(out)

    def estimate_frames(self, depth_images: torch.Tensor, masks: torch.Tensor, shape_optimization: bool = True,
                        prior_orientation_distribution: Optional[torch.Tensor] = None,
                        training_orientation_distribution: Optional[torch.Tensor] = None,
                        log_path: Optional[str] = None, animation_path: Optional[str] = None) -> tuple:
        """K DIFFERENT frames with one object each -- what a caller of the reference does with K
        ``pipeline(depth_k, mask_k, color_k)`` calls over a sequence or a dataset --, refined side by side as the K rows
        of ``estimate_objects``' loop (the same cached ``MultiObjectRenderAndCompare`` and initialisation: a loop built
        by either call serves the other).  The camera of every frame sits at the origin.

        depth_images (K,H,W): masked and far-field-clipped IN PLACE, as ``__call__`` does (pass a copy if the full
        depth is used afterwards); masks (K,H,W) bool.  prior_orientation_distribution (K,C) /
        training_orientation_distribution (C,): one row per frame.  Returns position (K,3), orientation (K,4), scale
        (K,), latent (K,L): row k follows ``estimate_objects(depth_images[k], masks[k][None])`` as that follows
        ``__call__`` (its docstring); K copies of one frame under K masks are ``estimate_objects(frame, masks)`` bit for
        bit.  ``best_estimates()`` works as after ``estimate_objects``.  ``ValueError`` for other shapes;
        ``NoDepthError`` for a frame without a valid pixel, raised AFTER the call's work was enqueued.
        log_path / animation_path: as in ``estimate_objects``."""
        self._no_step_files("estimate_frames", log_path, animation_path)
        if depth_images.dim() != 3 or tuple(masks.shape) != tuple(depth_images.shape):
            raise ValueError("depth_images (K,H,W) and masks (K,H,W) are expected, got "
                             f"{tuple(depth_images.shape)} and {tuple(masks.shape)}")
        K, H, W = (int(x) for x in depth_images.shape)
        if K < 1 or (H, W) != (int(self.cam.height), int(self.cam.width)):
            raise ValueError(f"depth_images of shape {(K, H, W)}: K >= 1 images of the camera's "
                             f"{int(self.cam.height)} x {int(self.cam.width)} pixels are expected")
        dev = self._dev
        loop = self._objects_loop(K, 1, shape_optimization)
        with torch.no_grad():
            if (depth_images.is_cuda and depth_images.dtype is torch.float32 and depth_images.is_contiguous()
                    and depth_images.device == dev):
                # one image per row already: preprocessed in place on the way into the loop's buffers
                loop.rebind(depth_images, masks=masks, far_field=self._far_field)
            else:     # any other tensor: the reference's two in-place assignments, then the copy
                depth_images[~masks.to(device=depth_images.device, dtype=torch.bool)] = 0
                if self._far_field is not None:
                    depth_images[depth_images > self._far_field] = 0
                loop.rebind(depth_images.to(dev, torch.float32).contiguous())
            return self._run_objects(loop, prior_orientation_distribution, training_orientation_distribution)

    # ---- N orientation hypotheses of one object ----------------------------------------------------------------
    def _hypothesis_loop(self, depth_images: torch.Tensor, masks: torch.Tensor, hypotheses: int,
                         camera_positions, camera_orientations, shape_optimization: bool):
        """the K-row loop with K = N rows for ONE object, bound to its V images (the masks repeated N times)"""
        N = int(hypotheses)
        if not 1 <= N <= _lib.ABI["SDFR_MAX_HYPOTHESES"]:
            raise ValueError(f"hypotheses must be in [1, {_lib.ABI['SDFR_MAX_HYPOTHESES']}], got {hypotheses}")
        if depth_images.dim() not in (2, 3) or tuple(masks.shape) != tuple(depth_images.shape):
            raise ValueError("depth_images (H,W) or (V,H,W) and the masks of ONE object in the same shape are expected")
        V = 1 if depth_images.dim() == 2 else int(depth_images.shape[0])
        # (the inlier bookkeeping always runs: it is the score; "hypotheses" keeps these loops apart from
        # estimate_objects' loops of the same K)
        key = ("hypotheses", N, bool(shape_optimization), V)

        def build():
            loop = MultiObjectRenderAndCompare(
                self.vae, self.cam, self.config, N, shape_optimization=shape_optimization, device=self._dev,
                sdf_grad_mode=self.sdf_grad_mode, views=V, track_inliers=True)
            f32 = dict(dtype=torch.float32, device=self._dev)
            loop.selection = dict(row=torch.zeros(loop.n, **f32), index=torch.zeros(1, dtype=torch.int32, device=self._dev),
                                  score=torch.zeros(1, **f32), initial=torch.zeros((N, loop.n), **f32))
            return loop

        loop = self._multi_loops.get_or_build(key, build)
        H, W = loop.H, loop.W
        with torch.no_grad():
            # (frames + masks: every row gets its own masked copy, the caller's depth is only read)
            loop.rebind(depth_images.reshape(V, H, W), camera_positions, camera_orientations,
                        masks=masks.reshape(1, V, H, W).expand(N, V, H, W), far_field=self._far_field)
        return loop

    def _refine_bound(self, loop: MultiObjectRenderAndCompare, position, orientation, scale, latent, index=None,
                      probability=None) -> tuple:
        """run the N rows of a bound loop and select: every launch on the current stream, nothing read back"""
        N, n = loop.K, loop.n
        sel = loop.selection
        with torch.no_grad():
            initial = sel["initial"]
            initial[:, 0:3] = position.reshape(N, 3)
            initial[:, 3:7] = orientation.reshape(N, 4)
            initial[:, 7] = scale.reshape(N)
            initial[:, 8:] = latent.reshape(N, loop.Lz)
            loop(initial[:, 0:3], initial[:, 3:7], initial[:, 7], initial[:, 8:])
            score, stride = self._hypothesis_scores(loop)
            _lib.check(loop.L.sdfr_select_row(score.data_ptr(), stride, N, loop.params.data_ptr(), n,
                                              sel["row"].data_ptr(), sel["index"].data_ptr(), sel["score"].data_ptr(),
                                              self._dev.index, torch.cuda.current_stream(self._dev).cuda_stream),
                       "sdfr_select_row")
            row = sel["row"]
            out = row[0:3][None].clone(), row[3:7][None].clone(), row[7:8].clone(), row[8:][None].clone()
        self._last_multi_loop = loop
        self._last_estimate = loop
        self._last_hypotheses = dict(loop=loop, index=index, probability=probability)
        return out

    def _hypothesis_scores(self, loop: MultiObjectRenderAndCompare):
        """(first score, stride in floats): every row's inlier ratio at the last iteration, or its best one with
        ``result_selection_strategy: best_inlier_ratio``; without an iteration all are 0 and row 0 wins"""
        if self.result_selection_strategy == "best_inlier_ratio":
            return loop.best_state[:, 0], 3
        last = max(loop.max_history - 1, 0)
        return loop.inlier_history[:, last], max(loop.max_history, 1)

    def refine_hypotheses(self, depth_images: torch.Tensor, masks: torch.Tensor, position: torch.Tensor,
                          orientation: torch.Tensor, scale: torch.Tensor, latent: torch.Tensor,
                          camera_positions: Optional[torch.Tensor] = None,
                          camera_orientations: Optional[torch.Tensor] = None, shape_optimization: bool = True) -> tuple:
        """N estimates of ONE object -- position (N,3), orientation (N,4), scale (N,), latent (N,L) -- refined side by
        side on the same observation (``MultiObjectRenderAndCompare`` with K = N rows, every row the object's own masked
        images), and the one the observation supports best: the largest inlier ratio (simple_setup.py:177-211, on the
        last view) at the last iteration, or each row's best ratio with ``result_selection_strategy:
        best_inlier_ratio``; equal ratios go to the smaller row, a NaN ratio (0 / 0: an image without a valid
        pixel) ranks below every number (``sdfr_select_row``, on the device).
        depth_images (H,W) or (V,H,W), NOT modified; masks: the object's, same shape.  Returns (position (1,3),
        orientation (1,4), scale (1,), latent (1,L)): the winner's LAST iterate, as ``__call__`` returns.  ``NoDepthError``
        is raised after the work was enqueued, as in ``estimate_objects``; ``last_hypotheses()`` has every row."""
        N = int(position.reshape(-1, 3).shape[0])
        loop = self._hypothesis_loop(depth_images, masks, N, camera_positions, camera_orientations, shape_optimization)
        out = self._refine_bound(loop, position, orientation, scale, latent)
        if bool((loop.counts == 0).any()):
            raise NoDepthError
        return out

    def estimate_hypotheses(self, depth_images: torch.Tensor, masks: torch.Tensor, color_images=None,
                            hypotheses: int = 1, camera_positions: Optional[torch.Tensor] = None,
                            camera_orientations: Optional[torch.Tensor] = None, shape_optimization: bool = True,
                            prior_orientation_distribution: Optional[torch.Tensor] = None,
                            training_orientation_distribution: Optional[torch.Tensor] = None) -> tuple:
        """``__call__`` with N starts instead of one: the initialisation network's estimate from the object's first view,
        once per each of the N most probable cells of its (prior-adjusted) orientation posterior
        (``ResidentInit(hypotheses=N)``), through ``refine_hypotheses``.  Where the argmax cell is wrong -- a symmetric
        body, a flat posterior, a hidden handle -- the loop converges into a wrong minimum from it; the other cells are
        the remedy the reference lacks.  Arguments as ``__call__`` (depth NOT modified; color_images unused); the prior
        is (C,) or (V,C), of which the first view's row counts.  Needs a discretized orientation head, the resident
        initialisation (no ``init_network`` override, ``resident_init=True``) and ``init_view: first`` for several views.
        ``hypotheses=1`` is ``estimate_objects(depth, mask[None])`` bit for bit."""
        N = int(hypotheses)
        if not 1 <= N <= _lib.ABI["SDFR_MAX_HYPOTHESES"]:
            raise ValueError(f"hypotheses (config key orientation_hypotheses) must be in "
                             f"[1, {_lib.ABI['SDFR_MAX_HYPOTHESES']}], got {hypotheses}")
        if (self._nn_init_override is not None or not isinstance(self.init_network, SDFPoseNet)
                or not self._resident_wanted):
            raise ValueError("orientation hypotheses are cells of the initialisation network's posterior: they need "
                             "the SDFPoseNet itself (no init_network override) and resident_init=True")
        if self.init_network.orientation_repr != "discretized":
            raise ValueError("orientation hypotheses need a discretized orientation head "
                             f"(init.head.orientation_repr: {self.init_network.orientation_repr})")
        V = 1 if depth_images.dim() == 2 else int(depth_images.shape[0])
        if V > 1 and self.config.get("init_view", "first") != "first":
            raise ValueError("orientation hypotheses with several views start from the first view (init_view: first), "
                             f"not init_view: {self.config.get('init_view')}")
        loop = self._hypothesis_loop(depth_images, masks, N, camera_positions, camera_orientations, shape_optimization)
        resident = self._resident_hypotheses.get_or_build(N, lambda: ResidentInit(
            self.init_network, self.cam, 1, dict(self.config, init_view="first"),
            normalize_pose=bool(self.init_config.get("normalize_pose", False)), hypotheses=N))
        with torch.no_grad():
            prior = prior_orientation_distribution
            if prior is not None:
                prior = prior.reshape(-1, resident.C)[0:1]
            # (on the loop's own address-stable buffers: row 0's first view, camera 0)
            resident(loop.target[0:1], loop.cam_pos[0:1], loop.cam_quat[0:1], prior, training_orientation_distribution)
            if N > 1:
                p, index, probability = resident.params_h, resident.hyp_index, resident.hyp_prob
            else:
                p, index, probability = resident.params[None], resident.index, resident.post_max
            out = self._refine_bound(loop, p[:, 0:3], p[:, 3:7], p[:, 7], p[:, 8:], index, probability)
            if resident.empty_views():
                raise NoDepthError
            if V > 1 and bool((loop.counts == 0).any()):
                raise NoDepthError
            if int(self.config.get("gauss_newton_iterations", 0)) > 0:
                # all N rows are refined; the winner stays the one the loop's inlier ratios selected
                self._gauss_newton(out)
                row = loop.params.index_select(0, loop.selection["index"].long())[0]
                out = row[0:3][None].clone(), row[3:7][None].clone(), row[7:8].clone(), row[8:][None].clone()
        return out

    def last_hypotheses(self):
        """the last ``estimate_hypotheses`` / ``refine_hypotheses`` call (also one routed from ``__call__``), read from
        the device here and nowhere else: ``index`` (N,) the cells and ``probability`` (N,) their posterior, descending
        (None after ``refine_hypotheses``, which is handed orientations, not cells), ``inlier_ratio`` (N,) the scores,
        ``winner`` the selected row, ``initial`` / ``final`` (N, 8 + L) the rows [position 3 | orientation 4 | scale |
        latent] before and after the loop.  None before the first such call."""
        last = self._last_hypotheses
        if last is None:
            return None
        loop = last["loop"]
        clone = lambda t: None if t is None else t.clone()
        return dict(index=clone(last["index"]), probability=clone(last["probability"]),
                    inlier_ratio=self._hypothesis_scores(loop)[0].clone(), winner=int(loop.selection["index"].item()),
                    initial=loop.selection["initial"].clone(), final=loop.params.clone())

    def pose_uncertainty(self, inlier_threshold=None, rcond: float = 1e-6, depth_sigma: Optional[float] = None):
        """How well the last call's observation determines its estimate (``sdfest_amd.uncertainty``): valid after
        ``__call__``, ``estimate_objects``, ``estimate_frames`` or ``estimate_hypotheses`` (``RuntimeError`` before any of
        them).  The reference returns a point estimate only and names an unobservable rotation in its metrics alone
        (rotational_symmetry_axis).

        From the last loop's bound targets and cameras and its final parameters: the final latents are decoded (the
        batched decode), the estimate is rendered (the forward), ONE ``sdfr_render_information`` call over all K V views
        gives every view's Gauss-Newton matrix of the depth residual, and each object's views are added in the WORLD
        tangent -- position (m), rotation vector (rad, ``q <- exp(w / 2) (x) q``), log-scale.  Returns
        ``uncertainty.PoseUncertainty`` with leading dimension K (1 after ``__call__``; the N rows after
        ``estimate_hypotheses``): information, covariance, sigma2, rank, position_std, rotation_std_deg, scale_rel_std,
        unobserved.  A direction the depth does not constrain (a symmetric body's spin) lowers ``rank`` and is listed in
        ``unobserved`` instead of being inverted.
        inlier_threshold: None = all overlap pixels; True = the pipeline's ``relative_inlier_threshold``; a number = that
        relative threshold (simple_setup.py:183-184).  rcond, depth_sigma: ``uncertainty.pose_covariance``.
        Reads the loop's buffers only: a following call returns what it would have returned."""
        from .uncertainty import pose_covariance, render_information, tangent_information
        thr = 0.0 if inlier_threshold is None else float(
            self._relative_inlier_threshold if inlier_threshold is True else inlier_threshold)
        with torch.no_grad():
            v = self._uncertainty_views()
            K, V = v["K"], v["V"]
            gram = render_information(v["depth"], v["target"], v["sdf"], v["position"], v["orientation"], v["inv_scale"],
                                      self.cam, thr)
            info = tangent_information(gram, v["orientation"], v["inv_scale"], v["camera_orientations"])
            per_object = lambda t: t.reshape((K, V) + tuple(t.shape[1:])).sum(dim=1)
            return pose_covariance(per_object(info), per_object(gram[:, 8, 8]), per_object(gram[:, 9, 9]), rcond=rcond,
                                   depth_sigma=depth_sigma)

    def _last_rows(self):
        """(loop, K, params (K, 8 + L)) of the last estimate: the loop that made it and its final parameter rows, a VIEW
        of the loop's own buffer -- what ``pose_uncertainty``, ``shape_uncertainty`` and ``refine`` start from"""
        loop = getattr(self, "_last_estimate", None)
        if loop is None:
            raise RuntimeError("pose_uncertainty() needs an estimate: call the pipeline (or estimate_objects, "
                               "estimate_frames, estimate_hypotheses) first")
        if isinstance(loop, MultiObjectRenderAndCompare):
            return loop, loop.K, loop.params
        if loop.group is not None:
            raise NotImplementedError("pose_uncertainty() after a loop sharded over ranks")
        return loop, 1, loop.params[None]

    def _uncertainty_views(self) -> Dict:
        """the K V views ``pose_uncertainty`` looks at, object-major (view k V + v is object k from camera v, as in the
        loops): the last loop's targets and cameras, its final parameters as camera-frame poses
        (pipeline.RenderAndCompare.losses), the decoded volumes and the rendered estimate"""
        from .differentiable_renderer import forward_raw
        from .lm import view_volumes
        loop, K, params = self._last_rows()
        V, cam_pos, cam_quat = loop.V, loop.cam_pos, loop.cam_quat
        H, W = int(self.cam.height), int(self.cam.width)
        with torch.no_grad():
            position, scale, latent = params[:, 0:3], params[:, 7], params[:, 8:]
            orientation = params[:, 3:7] / torch.linalg.norm(params[:, 3:7], dim=-1, keepdim=True)
            q_w2c = quaternion_invert(cam_quat)[None].expand(K, V, 4)
            pos_c = quaternion_apply(q_w2c, position[:, None, :] - cam_pos[None]).reshape(K * V, 3).contiguous()
            quat_c = quaternion_multiply(q_w2c, orientation[:, None, :].expand(K, V, 4)).reshape(K * V, 4).contiguous()
            inv_scale = (1.0 / scale)[:, None].expand(K, V).reshape(K * V).contiguous()
            sdf = self.vae.decode(latent.contiguous())[:, 0]
            # one object: its views share the grid; else every view its own copy
            sdf = view_volumes(sdf, K, V).contiguous()
            fx, fy, cx, cy, _ = self.cam.get_pinhole_camera_parameters(0.5)
            depth = forward_raw(sdf, pos_c, quat_c, inv_scale, W, H, cx, cy, fx, fy, self.config["threshold"])
        return dict(K=K, V=V, depth=depth, target=loop.target.reshape(K * V, H, W), sdf=sdf, position=pos_c,
                    orientation=quat_c, inv_scale=inv_scale,
                    camera_orientations=cam_quat[None].expand(K, V, 4).reshape(K * V, 4), latent=latent.contiguous())

    def _shape_uncertainty_views(self) -> Dict:
        """``_uncertainty_views`` plus the decoder's Jacobians at the K final latents: ``jac`` (K, D^3, Tp) as
        ``SDFDecoder.jvp`` writes it (the identity basis: T = the latent size) and ``jacobian``, what the K V views
        read -- the one buffer where a single object's views share it, else a copy per view, object-major like ``sdf``"""
        from .lm import view_volumes
        v = self._uncertainty_views()
        with torch.no_grad():
            _, jac = self.vae.decode_jvp(v["latent"])
        K, V = v["K"], v["V"]
        v["jac"], v["T"] = jac, int(v["latent"].shape[1])
        v["jacobian"] = view_volumes(jac, K, V)
        return v

    def shape_uncertainty(self, inlier_threshold=None, rcond: float = 1e-6, depth_sigma: Optional[float] = None,
                          latent_prior: float = 1.0, sdf_std: bool = False):
        """``pose_uncertainty`` without the assumption that the decoded shape is exact: the loop optimises the latent
        together with the pose and the two trade against each other (a mug seen from one side fits nearly as well a
        little larger and nearer), so the pose covariance conditioned on the shape is too small.  Valid after the same
        calls, with the same ``RuntimeError`` / ``NotImplementedError`` cases.

        The K final latents are decoded together with their Jacobian d SDF / d latent (``SDFVAE.decode_jvp``), ONE
        ``sdfr_render_information_shape`` call over all K V views gives every view's joint Gram matrix over pose and
        latent, and each object's views are added in the world tangent (the latent is frame-free).  Returns
        ``uncertainty.ShapePoseUncertainty`` with leading dimension K: the joint information and covariance, the pose
        covariance marginalised over the latent with position_std / rotation_std_deg / scale_rel_std from it,
        ``conditional`` (what ``pose_uncertainty`` reports), latent_std, rank, sigma2, unobserved.
        latent_prior: the weight of the VAE's N(0, I) prior on the latent (``uncertainty.shape_pose_covariance``; 0: none).
        sdf_std=True: also ``sdf_std`` (K, D, D, D), the standard deviation of every voxel of the decoded volume under
        the latent's covariance -- which part of the surface the observation pins down.
        Reads the loop's buffers only: a following call returns what it would have returned."""
        from . import uncertainty as U
        thr = 0.0 if inlier_threshold is None else float(
            self._relative_inlier_threshold if inlier_threshold is True else inlier_threshold)
        with torch.no_grad():
            v = self._shape_uncertainty_views()
            K, V, T = v["K"], v["V"], v["T"]
            gram = U.render_information(v["depth"], v["target"], v["sdf"], v["position"], v["orientation"],
                                        v["inv_scale"], self.cam, thr, jacobian=v["jacobian"], tangents=T)
            info = U.joint_tangent_information(gram, v["orientation"], v["inv_scale"], v["camera_orientations"])
            per_object = lambda t: t.reshape((K, V) + tuple(t.shape[1:])).sum(dim=1)
            rec = U.shape_pose_covariance(per_object(info), per_object(gram[:, 8 + T, 8 + T]),
                                          per_object(gram[:, 9 + T, 9 + T]), latent_prior=latent_prior, rcond=rcond,
                                          depth_sigma=depth_sigma)
            if sdf_std:
                rec.sdf_std = U.sdf_std(v["jac"], rec.covariance[:, 7:, 7:], tangents=T)   # (NaN where the row is)
            return rec

    def refine(self, iterations: int = 10, shape_optimization: Optional[bool] = None, inlier_threshold=None,
               latent_weight: float = 0.0, min_overlap: float = 0.5, pc_weight: Optional[float] = None, **lm):
        """Finish the last estimate by Levenberg-Marquardt on the squared depth residual (``sdfest_amd.lm``): valid after
        the same calls as ``pose_uncertainty``, with the same ``RuntimeError`` / ``NotImplementedError`` cases.  The loop is
        first order and returns the iterate Adam stopped at; the covariance ``pose_uncertainty`` / ``shape_uncertainty``
        report is that of the MINIMISER of the residual, and this takes the estimate there.  The reference has none.

        From the last loop's final parameters, bound targets and cameras: the start is evaluated, then `iterations` trials
        are judged, each one launch sequence on the current stream without an allocation or a host synchronisation
        (``LMRefiner``).  The refined rows are written back into that loop's parameters, so a following
        ``pose_uncertainty()`` / ``shape_uncertainty()`` is evaluated at them.
        shape_optimization: None = as the last call; False: the latent is not touched.  inlier_threshold: as
        ``pose_uncertainty``.  latent_weight: mu of the objective mean r^2 + mu |z|^2.  min_overlap: a trial keeping less
        than this share of the current pixels is rejected.  pc_weight: w > 0 adds the point-cloud term of the loop's
        objective, w mean r_pc^2 over the bound targets' back-projected points (``LMRefiner``); None reads the config key
        ``gauss_newton_pc_weight`` (default 0.0: the depth term alone, as before).  ``**lm``: ``lm.LM_DEFAULTS``.
        Returns ``((position (K,3), orientation (K,4) normalised, scale (K,), latent (K,L)), LMReport)``; the report is
        read back once, after the last iteration.  ``best_estimates()`` keeps reporting the Adam loop's bookkeeping."""
        from .lm import LMRefiner, _constants
        loop, K, params = self._last_rows()
        shape = bool(loop.shape_opt if shape_optimization is None else shape_optimization)
        thr = 0.0 if inlier_threshold is None else float(
            self._relative_inlier_threshold if inlier_threshold is True else inlier_threshold)
        w = float(self.config.get("gauss_newton_pc_weight", 0.0) if pc_weight is None else pc_weight)
        if not 0.0 <= w < float("inf"):
            raise ValueError(f"pc_weight = {w} must be finite and >= 0")
        # (a refiner with the point-cloud term owns more buffers: "pc on / off" is part of the key, the weight is not)
        refiner = self._refiners.get_or_build((K, int(loop.V), shape, w > 0.0), lambda: LMRefiner(
            self, K, int(loop.V), shape, device=self._dev, pc_weight=w))
        refiner.pc_weight = w
        refiner.inlier_threshold, refiner.latent_weight, refiner.min_overlap = thr, float(latent_weight), float(min_overlap)
        refiner.constants = _constants(lm)
        with torch.no_grad():
            refiner.start(params, loop.target, loop.cam_pos, loop.cam_quat)
            refiner.iterate(int(iterations) + 1)     # (the first one evaluates the start)
            params.copy_(refiner.params_cur)
            rows = refiner.params_cur.clone()
            orientation = rows[:, 3:7] / torch.linalg.norm(rows[:, 3:7], dim=-1, keepdim=True)
        self._last_refiner = refiner
        return (rows[:, 0:3], orientation, rows[:, 7], rows[:, 8:]), refiner.report()

    def _gauss_newton(self, estimate: tuple) -> tuple:
        """config key ``gauss_newton_iterations`` (default 0: `estimate` as it is): the estimation calls end with
        ``refine`` of that many iterations and return its rows; ``gauss_newton_pc_weight`` (default 0.0) is the weight of
        the point-cloud term in that refinement's objective"""
        n = int(self.config.get("gauss_newton_iterations", 0))
        return self.refine(n)[0] if n > 0 else estimate

    def best_estimates(self):
        """K entries (ratio, 1-based iteration, (position, orientation, scale, latent)), one per object: the parameters
        at each object's best inlier ratio in the last ``estimate_objects`` call (``result_selection_strategy ==
        "best_inlier_ratio"``); None when that call did not keep the bookkeeping"""
        loop = getattr(self, "_last_multi_loop", None)
        return loop.best_estimates() if loop is not None else None

    def prepare(self, views: int = 1, shape_optimization: bool = True) -> "SDFPipeline":
        """Optional: build the loop for `views` images and capture its graphs NOW (on an empty observation) instead of
        inside the first call -- a service that must answer its first request in the steady-state time calls this
        after construction.  The reference has no counterpart (it re-uses nothing between calls)."""
        loop = self._loop(views, shape_optimization)
        with torch.no_grad():
            H, W = self.cam.height, self.cam.width
            loop.rebind(torch.zeros((views, H, W), device=self._dev))
            z = torch.zeros((1, self.vae.latent_size), device=self._dev)
            loop(torch.tensor([[0.0, 0.0, -1.0]], device=self._dev), torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=self._dev),
                 torch.tensor([0.1], device=self._dev), z)
            resident = self._resident_init(views)
            if resident is not None:
                resident(loop.target, loop.cam_pos_all, loop.cam_quat_all)
            torch.cuda.synchronize(self._dev)
        return self

    def best_estimate(self):
        """(ratio, 1-based iteration, (position, orientation, scale, latent)) at the best inlier ratio of the last call
        (``result_selection_strategy == "best_inlier_ratio"``); None otherwise"""
        loop = getattr(self, "_last_loop", None)
        return loop.best_estimate() if loop is not None and loop.track_inliers else None
