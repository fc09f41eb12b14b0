"""Annotated Redwood dataset with its instance masks on the GPU: the interface and the files of the reference's
``sdfest/initialization/datasets/redwood_dataset.py::AnnotatedRedwoodDataset`` -- its config keys and defaults, class
attributes, directory layout, ``annotations.json`` and sample dictionary -- written anew around ``render_mesh_depth``
(the annotated mesh at its annotated pose) and ``visible_mask`` (``sdfr_visible_mask``), which replace the reference's
off-screen Open3D window and its boolean tensor passes per sample.

Expected directory format, as the reference's:
    {root_dir}/{category_str}/rgbd/{sequence_id}/rgb/{rgb_file}, .../depth/{depth_file}
    {ann_dir}/annotations.json      {sequence_id: {"mesh", "category", "scale", "pose_anns": [{"position",
                                    "orientation", "rgb_file", "depth_file"}]}}
    {ann_dir}/{mesh}

Differences from the reference:
  - ``category_str`` filters the samples, as the reference's docstring says (its code never applies the filter);
  - ``scale_convention``, ``orientation_repr``, the axis remapping, ``category_str`` and the camera are checked at
    construction, before any file is read, with the reference's error types (it fails at the first sample);
  - a sequence's mesh is read once and kept on the device; ``samples(indices)`` draws all requested frames with one
    raster call per distinct mesh and masks them with one call;
  - the camera and the occlusion margin are config keys (``camera``, ``occlusion_margin``), with the reference's
    constants (:144, :274) as defaults;
  - ``load_mesh`` returns this package's ``Mesh`` (device tensors), not an open3d ``TriangleMesh``.
"""
import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from PIL import Image

from .differentiable_renderer import Camera
from .mesh import Mesh, render_mesh_depth, visible_mask
from .nocs_dataset import matrix_to_quaternion, object_axes_matrix, read_depth
from .pipeline import quaternion_multiply
from .pointset_utils import (_CONVENTIONS, change_orientation_camera_convention, change_position_camera_convention,
                             depth_to_pointcloud, normalize_points)

_SCALES = {
    "diagonal": lambda extents: torch.linalg.norm(extents),        # what NOCS calls the scale
    "max": lambda extents: extents.max(),
    "half_max": lambda extents: 0.5 * extents.max(),
    "full": lambda extents: extents,
}


class AnnotatedRedwoodDataset(torch.utils.data.Dataset):
    """Dataset class for the annotated Redwood dataset (http://redwood-data.org/3dscan; the annotations are part of
    the SDFEst repository): real RGB-D frames with a ground-truth mesh and pose each.

    Config keys (``default_config``; see the reference's ``AnnotatedRedwoodDataset.Config`` for their meaning):
    root_dir, ann_dir, mask_pointcloud, normalize_pointcloud, scale_convention ("diagonal", "max", "half_max", "full"),
    camera_convention ("opengl", "opencv"), orientation_repr ("quaternion", "discretized"),
    orientation_grid_resolution, remap_y_axis, remap_x_axis, category_str.  Of this project: ``device``, ``camera``
    (keyword arguments of ``Camera``: the images' intrinsics) and ``occlusion_margin`` (metres in front of the mesh
    from which a depth reading counts as an occluder)."""

    num_categories = 3
    category_id_to_str = {0: "bottle", 1: "bowl", 2: "mug"}
    category_str_to_id = {v: k for k, v in category_id_to_str.items()}

    default_config = {
        "root_dir": None,
        "ann_dir": None,
        "mask_pointcloud": False,
        "normalize_pointcloud": False,
        "camera_convention": "opengl",
        "scale_convention": "half_max",
        "orientation_repr": "quaternion",
        "orientation_grid_resolution": None,
        "category_str": None,
        "remap_y_axis": None,
        "remap_x_axis": None,
    }
    own_config = {"device": "cuda", "camera": dict(width=640, height=480, fx=525, fy=525, cx=319.5, cy=239.5),
                  "occlusion_margin": 0.01}

    def __init__(self, config: dict) -> None:
        cfg = dict(self.default_config)
        cfg.update(self.own_config)
        cfg.update(config)
        self._config = cfg
        if cfg["scale_convention"] not in _SCALES:
            raise ValueError(f"Specified scale convention {cfg['scale_convention']} not supported.")
        if cfg["camera_convention"] not in _CONVENTIONS:
            raise ValueError(f"Unsupported camera convention {cfg['camera_convention']}.")
        if cfg["category_str"] is not None and cfg["category_str"] not in self.category_str_to_id:
            raise ValueError(f"Unsupported category_str {cfg['category_str']}.")
        remap = (cfg["remap_x_axis"], cfg["remap_y_axis"])
        if (remap[0] is None) != (remap[1] is None):
            raise ValueError("Either both or none of remap_{y,x}_axis have to be None.")
        self._object_axes = None if remap[0] is None else object_axes_matrix(*remap)
        self._orientation_grid = None
        if cfg["orientation_repr"] == "discretized":
            from .so3grid import SO3Grid
            self._orientation_grid = SO3Grid(cfg["orientation_grid_resolution"])
        elif cfg["orientation_repr"] != "quaternion":
            raise NotImplementedError(f"Orientation representation {cfg['orientation_repr']} is not supported.")
        margin = float(cfg["occlusion_margin"])
        if not (0.0 <= margin < float("inf")):
            raise ValueError(f"occlusion_margin={cfg['occlusion_margin']} must be >= 0 and finite")
        self._margin = margin
        self._camera = cfg["camera"] if isinstance(cfg["camera"], Camera) else Camera(**cfg["camera"])
        if self._camera.s != 0:
            raise ValueError(f"camera skew s={self._camera.s} is not supported (only s = 0)")
        self._root_dir, self._ann_dir = cfg["root_dir"], cfg["ann_dir"]
        if self._root_dir is None or self._ann_dir is None:
            raise ValueError("root_dir and ann_dir are required")
        self._device = torch.device(cfg["device"])
        self._meshes: Dict[str, Mesh] = {}      # mesh path -> the mesh as annotated, on the device
        self._load_annotations()

    camera = property(lambda self: self._camera)

    def __len__(self) -> int:
        return len(self._raw_samples)

    # ---- annotations -------------------------------------------------------------------------------------------------
    def _load_annotations(self) -> None:
        """the sample list: sequences in file order, their ``pose_anns`` in order; of one category with
        ``category_str``"""
        with open(os.path.join(self._ann_dir, "annotations.json"), "r") as f:
            anns = json.load(f)
        only = self._config["category_str"]
        self._raw_samples = []
        for seq_id, seq in anns.items():
            category = seq["category"]
            if category not in self.category_str_to_id:
                raise ValueError(f"Unsupported category {category} of sequence {seq_id}.")
            if only is not None and category != only:
                continue
            folder = os.path.join(self._root_dir, category, "rgbd", seq_id)
            for ann in seq["pose_anns"]:
                self._raw_samples.append({
                    "position": torch.tensor(ann["position"], dtype=torch.float32),
                    "orientation_q": torch.tensor(ann["orientation"], dtype=torch.float32),
                    "extents": torch.tensor(seq["scale"], dtype=torch.float32) * 2,
                    "color_path": os.path.join(folder, "rgb", ann["rgb_file"]),
                    "depth_path": os.path.join(folder, "depth", ann["depth_file"]),
                    "mesh_path": os.path.join(self._ann_dir, seq["mesh"]),
                    "category_str": category,
                })

    def annotation(self, idx: int) -> dict:
        """The pose part of sample `idx` (redwood_dataset.py:225-238, :284-365) as HOST tensors, without touching the
        GPU or the images: "position" (3,) in the configured camera convention (not shifted by
        ``normalize_pointcloud``: that needs the points), "quaternion" (4,) scalar-last, object (in the remapped axes)
        to camera, "orientation" (the quaternion, or its grid cell as int64), "scale" (() or (3,)), "extents" (3,) in
        the remapped axes, and "color_path", "depth_path", "obj_path", "category_id", "category_str"."""
        raw = self._raw_samples[idx]
        convention = self._config["camera_convention"]
        position = change_position_camera_convention(raw["position"], "opencv", convention)
        quaternion, extents = self._in_object_axes(raw["orientation_q"], raw["extents"])
        quaternion = change_orientation_camera_convention(quaternion, "opencv", convention)
        if self._orientation_grid is None:
            orientation = quaternion
        else:
            orientation = torch.tensor(self._orientation_grid.quat_to_index(quaternion.numpy()), dtype=torch.long)
        return {"position": position, "quaternion": quaternion, "orientation": orientation,
                "scale": torch.as_tensor(_SCALES[self._config["scale_convention"]](extents)), "extents": extents,
                "color_path": raw["color_path"], "depth_path": raw["depth_path"], "obj_path": raw["mesh_path"],
                "category_id": self.category_str_to_id[raw["category_str"]], "category_str": raw["category_str"]}

    def _in_object_axes(self, orientation_q: torch.Tensor, extents: torch.Tensor) -> tuple:
        """(quaternion, extents) for the remapped object axes; both unchanged without a remapping"""
        if self._object_axes is None:
            return orientation_q, extents
        axes = self._object_axes        # annotated object frame -> new object frame
        new_extents = (torch.as_tensor(axes, dtype=extents.dtype) @ extents).abs()
        # annotated: original object -> camera; wanted: new object -> original object -> camera
        back = torch.from_numpy(matrix_to_quaternion(axes.T))
        return quaternion_multiply(orientation_q, back), new_extents

    # ---- meshes ------------------------------------------------------------------------------------------------------
    def _mesh(self, path: str) -> Mesh:
        """the mesh file as annotated (metres, its own axes), read once"""
        mesh = self._meshes.get(path)
        if mesh is None:
            mesh = self._meshes[path] = Mesh.from_file(path, 1.0, rel_scale=True, center=False, device=self._device)
        return mesh

    def load_mesh(self, object_path: str) -> Mesh:
        """The object mesh in the configured object axes (redwood_dataset.py:390-403): a new ``Mesh`` at the identity
        pose whose vertices (and normals) are the file's, rotated by the axis remapping where there is one."""
        mesh = self._mesh(object_path)
        vertices, normals = mesh.vertices, mesh.normals
        if self._object_axes is not None:
            rotation = torch.as_tensor(self._object_axes, dtype=torch.float32, device=vertices.device)
            vertices = vertices @ rotation.T
            normals = None if normals is None else normals @ rotation.T
        return Mesh(vertices, mesh.faces, normals, scale=1.0, rel_scale=True)

    # ---- samples -----------------------------------------------------------------------------------------------------
    def __getitem__(self, idx: int) -> dict:
        """Sample: "color" (H,W,3), "depth" (H,W), "mask" (H,W) bool, "pointset" (N,3), "position" (3,),
        "orientation" (quaternion (4,) or the cell's index), "quaternion" (4,), "scale" (() or (3,)) -- tensors on the
        dataset's device -- and "color_path", "obj_path", "category_id", "category_str"."""
        return self.samples([idx])[0]

    def samples(self, indices: Sequence[int]) -> List[dict]:
        """``[self[i] for i in indices]``, bit for bit, with the frames' meshes drawn by one ``render_mesh_depth`` call
        per distinct mesh and all masks made by one ``visible_mask`` call."""
        indices = [int(i) for i in indices]
        if not indices:
            return []
        dev, camera = self._device, self._camera
        H, W = int(camera.height), int(camera.width)
        raws = [self._raw_samples[i] for i in indices]
        n = len(raws)
        observed = np.empty((n, H, W), dtype=np.float32)
        for k, raw in enumerate(raws):
            depth = read_depth(raw["depth_path"])
            if depth.shape != (H, W):
                raise ValueError(f"{raw['depth_path']}: a {depth.shape[1]} x {depth.shape[0]} image, the camera has "
                                 f"{W} x {H}")
            observed[k] = depth
        observed = torch.from_numpy(observed).to(dev)
        # the annotated poses are OpenCV poses of the mesh as it is in its file, whatever the sample's conventions
        positions = torch.stack([raw["position"] for raw in raws]).to(dev)
        orientations = torch.stack([raw["orientation_q"] for raw in raws]).to(dev)
        rendered = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        by_mesh: Dict[str, List[int]] = {}
        for k, raw in enumerate(raws):
            by_mesh.setdefault(raw["mesh_path"], []).append(k)
        for path, rows in by_mesh.items():
            whole = rows == list(range(n))
            out = render_mesh_depth(self._mesh(path), camera, positions[rows], orientations[rows], convention="open3d",
                                    out=rendered if whole else None)
            if not whole:
                rendered[rows] = out
        masks = visible_mask(rendered, observed, self._margin)
        return [self._sample(i, observed[k], masks[k]) for k, i in enumerate(indices)]

    def _sample(self, idx: int, depth: torch.Tensor, mask: torch.Tensor) -> dict:
        cfg, dev = self._config, self._device
        ann = self.annotation(idx)
        points = depth_to_pointcloud(depth, self._camera, mask=mask if cfg["mask_pointcloud"] else None,
                                     convention=cfg["camera_convention"])
        position = ann["position"].to(dev)
        if cfg["normalize_pointcloud"]:
            points, centroid = normalize_points(points)
            position = position - centroid
        color = np.asarray(Image.open(ann["color_path"]), dtype=np.float32) / 255
        return {"color": torch.from_numpy(color).to(dev), "depth": depth, "pointset": points, "mask": mask,
                "position": position, "orientation": ann["orientation"].to(dev), "quaternion": ann["quaternion"].to(dev),
                "scale": ann["scale"].to(dev), "color_path": ann["color_path"], "obj_path": ann["obj_path"],
                "category_id": ann["category_id"], "category_str": ann["category_str"]}

    # ---- the trainer's validation batches ----------------------------------------------------------------------------
    def validation_batches(self, batch_size: int, max_points: int = 2500, seed: int = 0) -> list:
        """[(points (n, M, 3), targets)] for ``SDFPoseNetTrainer.validate``, as ``NOCSDataset.validation_batches``:
        consecutive samples in batches of `batch_size` (one ``samples`` call each), every point set reduced to M =
        min(the batch's smallest set, max_points) points drawn without replacement by a host generator seeded with
        `seed`.  targets: "position", "scale", "orientation", "quaternion".  A Redwood sample has no latent."""
        gen = torch.Generator().manual_seed(int(seed))
        batches = []
        for first in range(0, len(self), batch_size):
            samples = self.samples(range(first, min(first + batch_size, len(self))))
            M = min(min(int(s["pointset"].shape[0]) for s in samples), int(max_points))
            if M < 1:
                raise ValueError("a sample without points cannot be collated")
            sets = [s["pointset"][torch.randperm(int(s["pointset"].shape[0]), generator=gen)[:M].to(self._device)]
                    for s in samples]
            targets = {k: torch.stack([s[k] for s in samples]) for k in ("position", "scale", "orientation", "quaternion")}
            # (a remapped quaternion is float64, as the reference's is: the trainer's tensors are float32)
            targets = {k: t.float() if t.is_floating_point() else t for k, t in targets.items()}
            batches.append((torch.stack(sets), targets))
        return batches
