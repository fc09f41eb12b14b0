"""The synthetic-view evaluation loop on the device: what the reference's
``estimation/scripts/rendering_evaluation.py`` does per mesh (``_generate_views``, ``_evaluate_file``,
``_compute_metric_stats``) -- depth images of a ground-truth mesh from random cameras, ``SDFPipeline`` on them, the
estimate's mesh, samples of both surfaces, the reconstruction metrics -- with this package's own stages
(``render_mesh_depth``, ``SDFPipeline``, ``generate_mesh``, ``sample_points``, ``evaluate_metrics``) and no host round
trip between them but the one the metrics end in.  Visualisation and logs are out of scope, as in ``simple_setup``.

``evaluate_annotated`` is the same loop over REAL frames with ground-truth poses and meshes (a dataset such as
``AnnotatedRedwoodDataset``): what the reference's ``estimation/configs/redwood_evaluation.yaml`` is the config of.
"""
import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .generated_views import sample_uniform_quaternions
from .mesh import Mesh, extract_mesh, render_mesh_depth, sample_points
from .init_network import NoDepthError
from .metrics import _Quat, correct_thresh, evaluate_metrics, iou_3d
from .pipeline import quaternion_apply, quaternion_invert, quaternion_multiply
from .pointset_utils import change_orientation_camera_convention, change_position_camera_convention
from .sdf_utils import mesh_to_sdf, normalized_mesh

__all__ = ["view_poses", "generate_views", "evaluate_mesh", "evaluate_meshes", "vae_reconstruction", "metric_stats",
           "evaluate_annotated", "DEFAULT_METRICS", "DEFAULT_POSE_THRESHOLDS"]

# the ``metrics:`` mapping of the reference's estimation/configs/rendering_evaluation.yaml
DEFAULT_METRICS = {
    "mean_accuracy": {"f": "sdfest.estimation.metrics.mean_accuracy", "kwargs": {}},
    "mean_completeness": {"f": "sdfest.estimation.metrics.mean_completeness", "kwargs": {}},
    "chamfer": {"f": "sdfest.estimation.metrics.symmetric_chamfer", "kwargs": {}},
    "completeness_0_01": {"f": "sdfest.estimation.metrics.completeness_thresh", "kwargs": {"threshold": 0.01}},
    "accuracy_0_01": {"f": "sdfest.estimation.metrics.accuracy_thresh", "kwargs": {"threshold": 0.01}},
}


def view_poses(camera_orientations: torch.Tensor, mesh_orientation: torch.Tensor,
               camera_distance: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The camera algebra of ``_generate_views`` (rendering_evaluation.py:207-231) for V cameras at once, on whatever
    device (and in whatever dtype) the inputs are.

    camera_orientations (V,4): OpenGL camera to world, scalar last.  mesh_orientation (4,): the mesh in the world; the
    mesh sits at the world's origin.  Returns
      camera_positions (V,3): the camera in the world, `camera_distance` away with the mesh on its principal axis;
      mesh_positions (V,3), mesh_orientations (V,4): the mesh in each camera's Open3D frame (x right, y down, z
      forward) -- the position is (0, 0, camera_distance)."""
    q = camera_orientations
    V = q.shape[0]
    back = q.new_tensor([0.0, 0.0, -float(camera_distance)]).expand(V, 3)
    camera_positions = -quaternion_apply(q, back)
    o3d_to_ogl = q.new_tensor([1.0, 0.0, 0.0, 0.0]).expand(V, 4)     # the half turn about x
    o3d_to_world = quaternion_multiply(q, o3d_to_ogl)
    mesh_orientations = quaternion_multiply(quaternion_invert(o3d_to_world), mesh_orientation.to(q).expand(V, 4))
    mesh_positions = q.new_tensor([0.0, 0.0, float(camera_distance)]).expand(V, 3).contiguous()
    return camera_positions, mesh_positions, mesh_orientations


def generate_views(mesh: Mesh, camera, num_views: int, camera_distance: float,
                   generator: Optional[torch.Generator] = None,
                   camera_orientations: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Random views around `mesh` (``_generate_views``): uniformly distributed camera orientations, every camera
    `camera_distance` from the mesh with the mesh on its principal axis, the mesh in its own world orientation at the
    world's origin (its ``position`` is set to zero, as the reference sets it).

    Returns the reference's dictionary, ready for ``SDFPipeline.__call__(**views)``: depth_images (V,H,W) float32,
    masks (V,H,W) bool (= depth != 0), color_images (V,H,W,3) zeros, camera_positions (V,3), camera_orientations (V,4)
    (OpenGL camera to world), all on the mesh's device.  All views are rendered by one ``render_mesh_depth`` call; a
    view in which no pixel sees the mesh is drawn again with a new orientation, as the reference draws it again (one
    host check per round of views, not per view).  camera_orientations (V,4): these orientations instead of random
    ones (a view that sees nothing is then an error)."""
    V = int(num_views)
    if V < 1:
        raise ValueError(f"num_views={num_views} must be >= 1")
    dev = mesh.vertices.device
    mesh.position = torch.zeros(3, device=dev)
    H, W = int(camera.height), int(camera.width)
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    cam_q = torch.empty((V, 4), dtype=torch.float32, device=dev)
    cam_p = torch.empty((V, 3), dtype=torch.float32, device=dev)
    todo = torch.arange(V, device=dev)
    if camera_orientations is not None and tuple(camera_orientations.shape) != (V, 4):
        raise ValueError(f"camera_orientations of shape {tuple(camera_orientations.shape)}: ({V},4) expected")
    for _ in range(100):
        if camera_orientations is not None:
            q = camera_orientations.detach().to(dev, torch.float32)
        else:
            q = sample_uniform_quaternions(int(todo.numel()), generator).to(dev)
        p, mesh_p, mesh_q = view_poses(q, mesh.orientation, camera_distance)
        d = render_mesh_depth(mesh, camera, mesh_p, mesh_q, convention="open3d")
        depth[todo], cam_q[todo], cam_p[todo] = d, q, p
        todo = todo[~(d != 0).flatten(1).any(1)]
        if todo.numel() == 0:       # the round's one host read
            break
        if camera_orientations is not None:
            raise ValueError(f"generate_views: views {todo.tolist()} of the given camera orientations see nothing")
    else:
        raise RuntimeError("generate_views: the mesh cannot be seen from camera_distance "
                           f"{camera_distance} (100 rounds of empty views)")
    return {"depth_images": depth, "masks": depth != 0,
            "color_images": torch.zeros((V, H, W, 3), dtype=torch.float32, device=dev),
            "camera_positions": cam_p, "camera_orientations": cam_q}


def evaluate_mesh(pipeline, gt_mesh: Mesh, num_views: int, camera_distance: float, samples: int, seed: int,
                  metrics_config: Optional[dict] = None, shape_optimization: bool = True,
                  generator: Optional[torch.Generator] = None, return_details: bool = False):
    """``_evaluate_file`` for a mesh already loaded (``Mesh.from_file(path, scale, rel_scale, center=True)``): views of
    `gt_mesh` -> ``pipeline(**views)`` -> ``pipeline.generate_mesh(latent, scale, complete_mesh=True)`` posed with the
    estimate -> `samples` points of both meshes in the world with one `seed` -> the metrics of `metrics_config` (the
    ``metrics:`` mapping of the reference's config; default: that of rendering_evaluation.yaml) as {name: float}.

    With `return_details` also a dictionary of the views, the estimate (position, orientation, scale, latent), the
    estimated mesh and both point sets."""
    metrics_config = DEFAULT_METRICS if metrics_config is None else metrics_config
    views = generate_views(gt_mesh, pipeline.cam, num_views, camera_distance, generator)
    # the pipeline masks its depth argument in place; the caller's views stay as rendered
    position, orientation, scale, latent = pipeline(**dict(views, depth_images=views["depth_images"].clone()),
                                                    shape_optimization=shape_optimization)
    out_mesh = pipeline.generate_mesh(latent, scale, True)
    if out_mesh is None:
        raise KeyError("evaluate_mesh: the pipeline's config has no iso_threshold, so it generates no mesh")
    out_mesh.position = position[0].detach()
    out_mesh.orientation = orientation[0].detach()
    gt_pts = sample_points([gt_mesh], samples, seed)[0]
    out_pts = sample_points([out_mesh], samples, seed)[0]
    metrics = evaluate_metrics(gt_pts, out_pts, metrics_config)
    if return_details:
        return metrics, {"views": views, "estimate": (position, orientation, scale, latent), "mesh": out_mesh,
                         "gt_points": gt_pts, "points": out_pts}
    return metrics


def vae_reconstruction(vae, gt_mesh: Mesh, samples: int, seed: int, metrics_config: Optional[dict] = None,
                       level: float = 0.0, cells_per_dim: int = 64, padding: int = 0, return_details: bool = False):
    """The shape prior's ceiling next to ``evaluate_mesh``: how well the VAE alone reproduces `gt_mesh`, with no views
    and no optimisation.  ``mesh_to_sdf(gt_mesh, cells_per_dim, padding)`` (the reference's framing: the volume the
    VAE was trained on) -> ``vae.prepare_input`` -> the encoder's means (no sample is drawn) -> ``vae.decode`` ->
    ``extract_mesh(..., level, complete=True)`` -> `samples` points of the ground truth in that same normalised frame
    (``normalized_mesh``) and of the reconstruction with one `seed` -> the metrics of `metrics_config` (default: that
    of rendering_evaluation.yaml).  `cells_per_dim` must be the VAE's ``sdf_size``.

    Returns ({name: float}, latent (1, latent_size)); with `return_details` also a dictionary of the input volume, the
    decoded volume, the reconstructed mesh and both point sets."""
    metrics_config = DEFAULT_METRICS if metrics_config is None else metrics_config
    R = int(cells_per_dim)
    with torch.no_grad():
        grid = mesh_to_sdf(gt_mesh, R, padding).view(1, 1, R, R, R)
        x = grid.clone() if return_details else grid
        vae.prepare_input(x)
        latent, _ = vae.encoder(x)
        recon = vae.decode(latent)
        out_mesh = extract_mesh(recon[0, 0], level, complete=True)
    gt_pts = sample_points([normalized_mesh(gt_mesh, R, padding)], samples, seed)[0]
    out_pts = sample_points([out_mesh], samples, seed)[0]
    metrics = evaluate_metrics(gt_pts, out_pts, metrics_config)
    if return_details:
        return metrics, latent, {"sdf": grid[0, 0], "reconstruction": recon[0, 0], "mesh": out_mesh,
                                 "gt_points": gt_pts, "points": out_pts}
    return metrics, latent


def metric_stats(metrics_list: List[Dict[str, float]]) -> Dict[str, Dict[str, float]]:
    """``_compute_metric_stats``: {name: {"mean", "var" (population), "std"}} over a list of metric dictionaries"""
    stats = {}
    n = len(metrics_list)
    for name in (metrics_list[0] if metrics_list else {}):
        vals = [float(m[name]) for m in metrics_list]
        mean = sum(vals) / n
        var = sum((v - mean) ** 2 for v in vals) / n
        stats[name] = {"mean": mean, "var": var, "std": math.sqrt(var)}
    return stats


def evaluate_meshes(pipeline, gt_meshes: List[Mesh], num_views: int, camera_distance: float, samples: int, seed: int,
                    metrics_config: Optional[dict] = None, shape_optimization: bool = True,
                    generator: Optional[torch.Generator] = None) -> Dict[str, Dict[str, float]]:
    """``evaluate_mesh`` over a list of ground-truth meshes: the per-metric mean / var / std the reference's
    ``_compute_metric_stats`` returns"""
    return metric_stats([evaluate_mesh(pipeline, m, num_views, camera_distance, samples, seed, metrics_config,
                                       shape_optimization, generator) for m in gt_meshes])


# ---- annotated real frames -------------------------------------------------------------------------------------------
# name -> (degrees, metres): the four usual pairs
DEFAULT_POSE_THRESHOLDS = {"5deg_2cm": (5.0, 0.02), "5deg_5cm": (5.0, 0.05), "10deg_2cm": (10.0, 0.02),
                           "10deg_5cm": (10.0, 0.05)}


def pose_errors(position_gt, orientation_gt, position, orientation,
                rotational_symmetry_axis: Optional[int] = None) -> Tuple[float, float]:
    """(position error in metres, rotation error in degrees) of an estimate against the ground truth, in float64 on the
    host, by ``correct_thresh``'s formulas: the Euclidean distance; the angle of gt * estimate^-1, or, with a
    `rotational_symmetry_axis` (0, 1, 2), the angle between the two images of that object axis."""
    host = lambda v: np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1)
    position_error = float(np.linalg.norm(host(position_gt) - host(position)))
    r_gt, r = _Quat(host(orientation_gt)), _Quat(host(orientation))
    if rotational_symmetry_axis is None:
        radians = (r_gt * r.inv()).magnitude()
    else:
        axis = np.zeros(3)
        axis[int(rotational_symmetry_axis)] = 1.0
        radians = float(np.arccos(np.clip(r_gt.apply(axis) @ r.apply(axis), -1.0, 1.0)))
    return position_error, float(np.degrees(radians))


def _annotated_groups(dataset, indices: List[int], pipelines, frames_per_call: int, skipped: list) -> List[List[int]]:
    """runs of at most `frames_per_call` consecutive samples of one category; a sample whose category has no pipeline
    goes to `skipped` and ends a run"""
    groups, run, run_category = [], [], None
    for i in indices:
        category = dataset.annotation(i)["category_str"] if hasattr(dataset, "annotation") else dataset[i]["category_str"]
        if isinstance(pipelines, dict) and category not in pipelines:
            skipped.append({"index": i, "category_str": category, "reason": f"no pipeline for category {category}"})
            category = None
        if run and (category != run_category or len(run) >= frames_per_call):
            groups.append(run)
            run = []
        if category is not None:
            run.append(i)
        run_category = category
    if run:
        groups.append(run)
    return groups


def evaluate_annotated(pipelines, dataset, samples: int, seed: int, metrics_config: Optional[dict] = None,
                       pose_thresholds: Optional[dict] = None, symmetry_axes: Optional[dict] = None,
                       frames_per_call: int = 1, shape_optimization: bool = True,
                       indices: Optional[List[int]] = None, iou_thresholds: Optional[dict] = None) -> dict:
    """The evaluation over annotated real frames: every sample of `dataset` (``AnnotatedRedwoodDataset``, or anything
    with its sample dictionary, ``load_mesh`` and ``_config``) -> the pipeline on a clone of its depth under its mask
    -> ``pipeline.generate_mesh(latent, scale, True)`` posed with the estimate, and ``dataset.load_mesh(obj_path)``
    posed with the annotation -> `samples` points of each with one `seed` -> the metrics of `metrics_config`
    (default: ``DEFAULT_METRICS``) on the two point sets, the position error (metres) and the rotation error (degrees)
    in float64 on the host (``pose_errors``), and one ``correct_thresh`` flag per entry of `pose_thresholds` ({name:
    (degrees, metres)}; default ``DEFAULT_POSE_THRESHOLDS``).

    pipelines: one pipeline for every sample, or {category_str: pipeline}.  Only ``pipeline(depth, mask, color,
    shape_optimization=...)``, ``pipeline.generate_mesh`` and, for `frames_per_call` > 1, ``pipeline.estimate_frames``
    are used.  The dataset may use either camera convention: its poses are brought to the pipeline's OpenGL frame.
    symmetry_axes: {category_str: 0 | 1 | 2}, the ``rotational_symmetry_axis`` of such a category's rotation error and
    flags.  frames_per_call = K: runs of up to K consecutive samples of one category go through ``estimate_frames``
    together (a run in which a frame has no depth is done again frame by frame).  indices: these samples, in this
    order (default: all).  iou_thresholds: {name: IoU}, e.g. {"iou25": 0.25, "iou50": 0.5} -- every sample also gets
    "iou_3d", the 3D IoU (``metrics.iou_3d``; the category's symmetry axis applies) of the annotated box (the frame's
    "extents", or ``dataset.annotation(i)["extents"]``, at the ground-truth pose) and the estimate's
    (``out_mesh.oriented_box`` of the mesh generated anyway, at the estimate's pose in the precision the pipeline returned
    it), one "correct" flag per entry (IoU >= the threshold), "stats" the IoU's and the top-level "correct" the flags'
    shares;
    None (default): none of these, the result is what it was without the argument.

    Returns {"samples": [{"index", "category_str", "metrics": {name: float}, "position_error", "rotation_error",
    "correct": {name: 0 | 1}}], "stats": {category_str and "all": ``metric_stats`` of the metrics and the two errors},
    "correct": {name: the share of samples with the flag}, "skipped": [{"index", "category_str", "reason"}]} -- a sample
    whose category has no pipeline, or whose masked depth is empty (``NoDepthError``), is skipped."""
    metrics_config = DEFAULT_METRICS if metrics_config is None else metrics_config
    pose_thresholds = DEFAULT_POSE_THRESHOLDS if pose_thresholds is None else pose_thresholds
    symmetry_axes = {} if symmetry_axes is None else symmetry_axes
    K = int(frames_per_call)
    if K < 1:
        raise ValueError(f"frames_per_call={frames_per_call} must be >= 1")
    config = getattr(dataset, "_config", {})
    if config.get("normalize_pointcloud", False):
        raise ValueError("evaluate_annotated needs a dataset with normalize_pointcloud: False (a normalised sample's "
                         "position is shifted by its point cloud's centroid)")
    convention = config.get("camera_convention", "opengl")
    indices = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
    skipped, entries = [], {}
    for group in _annotated_groups(dataset, indices, pipelines, K, skipped):
        frames = dataset.samples(group) if hasattr(dataset, "samples") else [dataset[i] for i in group]
        category = frames[0]["category_str"]
        pipeline = pipelines[category] if isinstance(pipelines, dict) else pipelines
        estimates = None
        if len(frames) > 1:
            try:
                rows = pipeline.estimate_frames(torch.stack([f["depth"] for f in frames]),
                                                torch.stack([f["mask"] for f in frames]),
                                                shape_optimization=shape_optimization)
                estimates = [tuple(r[k:k + 1] for r in rows) for k in range(len(frames))]
            except NoDepthError:
                estimates = None      # which frame is empty is not known: one by one below
        for k, (i, frame) in enumerate(zip(group, frames)):
            if estimates is not None:
                estimate = estimates[k]
            else:
                try:     # the pipeline masks its depth argument in place; the sample stays as loaded
                    estimate = pipeline(frame["depth"].clone(), frame["mask"], frame["color"],
                                        shape_optimization=shape_optimization)
                except NoDepthError:
                    skipped.append({"index": i, "category_str": category, "reason": "no valid depth under the mask"})
                    continue
            entries[i] = _annotated_entry(pipeline, dataset, i, frame, estimate, convention, samples, seed,
                                          metrics_config, pose_thresholds, symmetry_axes.get(category), iou_thresholds)
    done = [entries[i] for i in indices if i in entries]
    rows = lambda es: [dict(e["metrics"], position_error=e["position_error"], rotation_error=e["rotation_error"],
                            **({"iou_3d": e["iou_3d"]} if iou_thresholds is not None else {})) for e in es]
    stats = {c: metric_stats(rows([e for e in done if e["category_str"] == c]))
             for c in dict.fromkeys(e["category_str"] for e in done)}
    stats["all"] = metric_stats(rows(done))
    correct = {name: (sum(e["correct"][name] for e in done) / len(done) if done else float("nan"))
               for name in list(pose_thresholds) + list(iou_thresholds or {})}
    order = {i: n for n, i in enumerate(indices)}
    return {"samples": done, "stats": stats, "correct": correct,
            "skipped": sorted(skipped, key=lambda s: order[s["index"]])}


def _annotated_entry(pipeline, dataset, index: int, frame: dict, estimate: tuple, convention: str, samples: int,
                     seed: int, metrics_config: dict, pose_thresholds: dict, symmetry_axis: Optional[int],
                     iou_thresholds: Optional[dict] = None) -> dict:
    position, orientation, scale, latent = estimate
    out_mesh = pipeline.generate_mesh(latent, scale, True)
    if out_mesh is None:
        raise KeyError("evaluate_annotated: the pipeline's config has no iso_threshold, so it generates no mesh")
    out_mesh.position = position[0].detach()
    out_mesh.orientation = orientation[0].detach()
    gt_position = change_position_camera_convention(frame["position"], convention, "opengl")
    gt_orientation = change_orientation_camera_convention(frame["quaternion"], convention, "opengl")
    gt_mesh = dataset.load_mesh(frame["obj_path"])
    gt_mesh.position = gt_position
    gt_mesh.orientation = gt_orientation
    gt_pts = sample_points([gt_mesh], samples, seed)[0]
    out_pts = sample_points([out_mesh], samples, seed)[0]
    metrics = evaluate_metrics(gt_pts, out_pts, metrics_config)
    position_error, rotation_error = pose_errors(gt_position, gt_orientation, position[0], orientation[0],
                                                 symmetry_axis)
    correct = {name: int(correct_thresh(gt_position, position[0], gt_orientation, orientation[0],
                                        position_threshold=metres, degree_threshold=degrees,
                                        rotational_symmetry_axis=symmetry_axis))
               for name, (degrees, metres) in pose_thresholds.items()}
    entry = {"index": index, "category_str": frame["category_str"], "metrics": metrics,
             "position_error": position_error, "rotation_error": rotation_error, "correct": correct}
    if iou_thresholds is not None:
        # (the estimate's pose as the pipeline returned it: the mesh's own pose attributes are float32)
        center, box_orientation, extents = out_mesh.oriented_box(position[0], orientation[0])
        # (the annotation's side lengths: a sample of AnnotatedRedwoodDataset carries its "scale" only)
        gt_extents = frame["extents"] if "extents" in frame else dataset.annotation(index)["extents"]
        entry["iou_3d"] = iou_3d(gt_position, gt_orientation, gt_extents, center, box_orientation, extents,
                                 rotational_symmetry_axis=symmetry_axis)
        for name, threshold in iou_thresholds.items():
            correct[name] = int(entry["iou_3d"] >= threshold)
    return entry
