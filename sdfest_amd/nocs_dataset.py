"""NOCS dataset (CAMERA / REAL) with its pose annotation on the GPU: the interface and the files of the reference's
``sdfest/initialization/datasets/nocs_dataset.py::NOCSDataset`` -- its config keys and defaults, class attributes,
preprocessing files and sample dictionary -- written anew around ``sdfr_nocs_correspondences`` (once per frame) and
``sdfr_similarity_ransac`` (once per batch of frames; sdfest_amd/nocs_utils.py), which replace the reference's
one-core numpy alignment of every annotated object's NOCS points to its depth points.

Differences from the reference:
  - the RANSAC's samples come from this project's Philox stream (key: ``seed``, the frame's number and the mask id), not
    from numpy's global stream: an object's annotation does not depend on which objects were annotated before it;
  - a frame's back-projection multiplies by the fp32 reciprocal focal length (this project's depth_to_pointcloud) where
    the reference's CPU tensors divide: the last bit of a target coordinate may differ;
  - ``_fix_obj_models`` (png textures named .jpg) is not needed: textures are never read, extents come from the OBJ's
    vertices (``Mesh.from_file``);
  - frames are decoded with PIL by a thread pool of at most 16 workers;
  - a split is preprocessed into ``{split}.partial`` and renamed to ``{split}`` when it is complete, so a run that dies
    midway leaves nothing a later construction would take for a finished split;
  - a frame's files are named from the colour file's stem (``0000_`` + ``depth.png``, ...), so a root directory whose own
    name contains "color" works;
  - ``scale_convention``, ``orientation_repr``, the axis remapping and ``category_str`` are checked at construction,
    before any preprocessing, with the reference's error types (it fails at the first sample);
  - a mask id without a row in the frame's meta file: the warning is the reference's, and, as there, the run fails
    (``IndexError``, named for what it is, where the reference fails on the empty match's first row).
The pickles carry the reference's keys and types, so either implementation reads what the other wrote.
"""
import glob
import json
import os
import pickle
import shutil
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List, NamedTuple, Optional

import numpy as np
import torch
from PIL import Image

from . import nocs_utils
from .differentiable_renderer import Camera
from .nocs_utils import PoseEstimationError
from .pipeline import quaternion_multiply
from .pointset_utils import (change_orientation_camera_convention, change_position_camera_convention,
                             depth_to_pointcloud, normalize_points)

COLOR_SUFFIX = "color.png"      # a frame is {stem}color.png, {stem}mask.png, {stem}coord.png, {stem}meta.txt, ...


class ObjectError(Exception):
    """Error if something with the mesh is wrong."""


class SplitLayout(NamedTuple):
    """Where a split's files are, below root_dir, and how it is annotated."""
    frames: str                 # folder of the colour / mask / coord / meta files
    depth_root: Optional[str]   # folder that mirrors `frames` with the depth images (None: next to the colour file)
    depth_name: str             # {stem}{depth_name}.png
    models: str                 # folder below obj_models
    shapenet_models: bool       # obj_models/{models}/{synset}/{object}/model.obj, unit diagonal; else {name}.obj, metric
    gts: Optional[str]          # folder below gts whose pickles hold the poses (None: estimated from the NOCS map)
    intrinsics: dict


# intrinsics: detect_eval.py of https://github.com/hughw19/NOCS_CVPR2019
_REAL = dict(width=640, height=480, fx=591.0125, fy=590.16775, cx=322.525, cy=244.11084, pixel_center=0.0)
_CAMERA = dict(width=640, height=480, fx=577.5, fy=577.5, cx=319.5, cy=239.5, pixel_center=0.0)
SPLITS = {
    "camera_train": SplitLayout("train", "camera_full_depths", "composed", "train", True, None, _CAMERA),
    "camera_val": SplitLayout("val", "camera_full_depths", "composed", "val", True, None, _CAMERA),
    "real_train": SplitLayout("real_train", None, "depth", "real_train", False, None, _REAL),
    # the ground truth poses are used for REAL test data only (those of CAMERA val contain errors)
    "real_test": SplitLayout("real_test", None, "depth", "real_test", False, "real_test", _REAL),
}

_SIGNED_AXES = {"x": (1.0, 0.0, 0.0), "y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0),
                "-x": (-1.0, 0.0, 0.0), "-y": (0.0, -1.0, 0.0), "-z": (0.0, 0.0, -1.0)}
_SCALES = {
    "diagonal": lambda record, extents: record["nocs_scale"],        # what NOCS itself calls the scale
    "max": lambda record, extents: record["max_extent"],
    "half_max": lambda record, extents: 0.5 * record["max_extent"],
    "full": lambda record, extents: extents,
}
_RECORD_TENSORS = ("nocs_transform", "position", "orientation_q", "extents")


def matrix_to_quaternion(m) -> np.ndarray:
    """Scalar-last unit quaternion of a rotation matrix, float64 (Shepperd's method: the largest of the trace and the
    diagonal entries picks the branch, as scipy's ``Rotation.from_matrix(m).as_quat()`` does)."""
    m = np.asarray(m, dtype=np.float64)
    d = np.array([m[0, 0], m[1, 1], m[2, 2], m[0, 0] + m[1, 1] + m[2, 2]])
    c = int(np.argmax(d))
    q = np.empty(4)
    if c == 3:
        q[0], q[1], q[2], q[3] = m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1 + d[3]
    else:
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q[i] = 1 - d[3] + 2 * m[i, i]
        q[j] = m[j, i] + m[i, j]
        q[k] = m[k, i] + m[i, k]
        q[3] = m[k, j] - m[j, k]
    return q / np.linalg.norm(q)


def read_meta(meta_path: str) -> list:
    """rows of a ``*_meta.txt``: [mask id (int), category id (int), further columns (str)...]"""
    rows = []
    with open(meta_path) as f:
        for line in f:
            parts = line.split()
            if parts:
                rows.append([int(parts[0]), int(parts[1])] + parts[2:])
    return rows


def object_axes_matrix(remap_x_axis: str, remap_y_axis: str) -> np.ndarray:
    """(3,3) rotation from the NOCS object frame to the one in which the NOCS x axis points along `remap_x_axis` and
    the NOCS y axis along `remap_y_axis` ("x", "-x", "y", ...): these are its first two columns, and the third is
    their cross product, so the frame stays right-handed.  ValueError for an unknown name or two parallel axes."""
    for key, name in (("remap_x_axis", remap_x_axis), ("remap_y_axis", remap_y_axis)):
        if name not in _SIGNED_AXES:
            raise ValueError(f"Unsupported {key} {name}")
    to_x, to_y = np.array(_SIGNED_AXES[remap_x_axis]), np.array(_SIGNED_AXES[remap_y_axis])
    to_z = np.cross(to_x, to_y)
    if not to_z.any():
        raise ValueError(f"remap_x_axis {remap_x_axis} and remap_y_axis {remap_y_axis} are the same axis")
    return np.stack([to_x, to_y, to_z], axis=1) + 0.0      # (+ 0.0: no negative zeros)


def pose_from_similarity_matrix(matrix) -> tuple:
    """(position (3,), rotation (3,3), scale) of a (4,4) similarity transform, the way the reference takes a stored
    ground truth pose apart: the scale is the first column's norm, and ROW i of the upper block is divided by the norm
    of COLUMN i -- the rotation itself for the uniform scale such a transform has."""
    matrix = np.asarray(matrix)
    block = matrix[:3, :3]
    norms = np.sqrt((block * block).sum(axis=0))
    return matrix[:3, 3], block / norms.reshape(3, 1), norms[0]


def read_instance_ids(mask_path: str) -> np.ndarray:
    """(H,W) uint8 instance ids, 255 for the background.  REAL masks are one-channel images; CAMERA masks are RGBA with
    the ids in the first channel."""
    image = np.asarray(Image.open(mask_path), dtype=np.uint8)
    return np.array(image if image.ndim == 2 else image[:, :, 0])      # (a contiguous copy the caller owns)


def read_depth(depth_path: str) -> np.ndarray:
    """(H,W) float32 metres of a 16-bit millimetre image"""
    return np.asarray(Image.open(depth_path), dtype=np.float32) * 0.001


class NOCSDataset(torch.utils.data.Dataset):
    """Dataset class for the NOCS datasets (CAMERA*, REAL*; CAMERA25 and REAL275 are the test data).

    Expected directory format, as the reference's: {root_dir}/real_train, real_test, gts, obj_models,
    camera_full_depths, val, train.  The first construction for a split preprocesses it into
    {root_dir}/sdfest_pre/{split}/{image_id:08}_{counter}.pkl and categories.json; later ones read those.

    Config keys (``default_config``; see the reference's ``NOCSDataset.Config`` for their meaning): root_dir, split
    ("camera_train", "camera_val", "real_train", "real_test"), mask_pointcloud, normalize_pointcloud, scale_convention
    ("diagonal", "max", "half_max", "full"), camera_convention ("opengl", "opencv"), orientation_repr ("quaternion",
    "discretized"), orientation_grid_resolution, remap_y_axis, remap_x_axis, category_str.  Of this project:
    ``seed`` (the RANSAC's sample stream), ``preprocess_batch`` (frames per fit launch), ``device``."""

    num_categories = 7
    category_id_to_str = {0: "unknown", 1: "bottle", 2: "bowl", 3: "camera", 4: "can", 5: "laptop", 6: "mug"}
    category_str_to_id = {v: k for k, v in category_id_to_str.items()}

    default_config = {
        "root_dir": None,
        "split": None,
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
    own_config = {"seed": 0, "preprocess_batch": 64, "device": "cuda"}

    def __init__(self, config: dict) -> None:
        cfg = dict(self.default_config)
        cfg.update(self.own_config)
        cfg.update(config)
        self._config = cfg
        if cfg["split"] not in SPLITS:
            raise ValueError(f"Specified split {cfg['split']} is not supported.")
        if cfg["scale_convention"] not in _SCALES:
            raise ValueError(f"Specified scale convention {cfg['scale_convention']} not supported.")
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
        self._root_dir = cfg["root_dir"]
        self._split = cfg["split"]
        self._layout = SPLITS[self._split]
        self._camera = Camera(**self._layout.intrinsics)
        self._device = torch.device(cfg["device"])
        self._seed = int(cfg["seed"])
        self._preprocess_batch = max(1, int(cfg["preprocess_batch"]))
        self._preprocess_path = os.path.join(self._root_dir, "sdfest_pre", self._split)
        self.preprocess_stats = None
        if not os.path.isdir(self._preprocess_path):
            self._preprocess_dataset()
        self._sample_files = self._list_samples(self._preprocess_path, cfg["category_str"])

    def __len__(self) -> int:
        return len(self._sample_files)

    def __getitem__(self, idx: int) -> dict:
        """Sample: "color" (H,W,3), "depth" (H,W), "mask" (H,W) bool, "pointset" (N,3), "position" (3,),
        "orientation" (quaternion (4,) or the cell's index), "quaternion" (4,), "scale" (() or (3,)) -- tensors on the
        dataset's device -- and "color_path", "obj_path", "category_id", "category_str"."""
        with open(self._sample_files[idx], "rb") as f:
            return self._sample_from_sample_data(pickle.load(f))

    # ---- preprocessing -------------------------------------------------------------------------------------------
    def _preprocess_dataset(self) -> None:
        """One file per annotated object, {image_id:08}_{counter}.pkl, and categories.json (category name -> file
        names).  Everything is written below {split}.partial, which becomes {split} with the last step.
        ``preprocess_stats`` afterwards: frames, objects, skipped, seconds, per-category counts."""
        started = time.time()
        partial = self._preprocess_path + ".partial"
        if os.path.isdir(partial):      # what a run that died left behind
            shutil.rmtree(partial)
        os.makedirs(partial)
        color_paths = sorted(glob.glob(os.path.join(self._root_dir, self._layout.frames, "**", "*_" + COLOR_SUFFIX),
                                       recursive=True))
        stats = {"frames": len(color_paths), "objects": 0, "skipped": 0}
        by_category = {name: [] for name in self.category_id_to_str.values()}
        step = self._preprocess_batch
        with ThreadPoolExecutor(max_workers=min(16, step, max(1, len(color_paths)))) as pool:
            for first in range(0, len(color_paths), step):
                numbered = list(enumerate(color_paths[first:first + step], start=first))
                frames = [f for f in pool.map(lambda pair: self._load_frame(*pair), numbered) if f is not None]
                for file_name, category_id in self._annotate_frames(frames, partial, stats):
                    by_category[self.category_id_to_str[category_id]].append(file_name)
        with open(os.path.join(partial, "categories.json"), "w") as f:
            json.dump({name: sorted(files) for name, files in by_category.items()}, f)
        os.rename(partial, self._preprocess_path)
        stats["seconds"] = time.time() - started
        stats["categories"] = {name: len(files) for name, files in by_category.items()}
        self.preprocess_stats = stats
        print(f"Finished preprocessing for {self._split}.")

    def _frame_file(self, color_path: str, name: str) -> str:
        """the file `name` ("mask.png", "meta.txt", ...) of the frame whose colour image is color_path"""
        return color_path[:-len(COLOR_SUFFIX)] + name

    def _depth_path(self, color_path: str) -> str:
        depth_path = self._frame_file(color_path, self._layout.depth_name + ".png")
        if self._layout.depth_root is None:
            return depth_path
        return os.path.join(self._root_dir, self._layout.depth_root, os.path.relpath(depth_path, self._root_dir))

    def _gts_path(self, color_path: str) -> str:
        """gts/{folder}/results_{frames folder}_{scene}_{frame number}.pkl"""
        frames, scene, file_name = os.path.normpath(color_path).split(os.sep)[-3:]
        number = file_name[:-len("_" + COLOR_SUFFIX)]
        return os.path.join(self._root_dir, "gts", self._layout.gts, f"results_{frames}_{scene}_{number}.pkl")

    def _obj_path(self, meta_row: list) -> str:
        models = os.path.join(self._root_dir, "obj_models", self._layout.models)
        if self._layout.shapenet_models:        # meta row: mask id, category, synset id, object id
            return os.path.join(models, meta_row[2], meta_row[3], "model.obj")
        return os.path.join(models, meta_row[2] + ".obj")       # mask id, category, object name

    def _load_frame(self, image_id: int, color_path: str) -> Optional[dict]:
        """Host side of a frame (a pool thread): decoded images, meta rows, the objects to annotate."""
        depth_path = self._depth_path(color_path)
        if not os.path.isfile(depth_path):
            print(f"Missing depth file {depth_path}. Skipping.")
            return None
        mask_path = self._frame_file(color_path, "mask.png")
        meta_path = self._frame_file(color_path, "meta.txt")
        meta = read_meta(meta_path)
        mask = read_instance_ids(mask_path)
        objects = []
        for mask_id in np.unique(mask).tolist():
            if mask_id == 255:       # background
                continue
            match = [row for row in meta if row[0] == mask_id]
            if not match:
                print(f"Warning: mask {mask_id} not found in {meta_path}")
                raise IndexError(f"mask id {mask_id} of {mask_path} has no row in {meta_path}")
            if len(match) != 1:
                print(f"Warning: mask {mask_id} not unique in {meta_path}")
            if match[0][1] == 0:     # unknown / distractor object
                continue
            objects.append((mask_id, match[0]))
        frame = dict(image_id=image_id, color_path=color_path, depth_path=depth_path, mask_path=mask_path, mask=mask,
                     objects=objects)
        if not objects:
            return frame
        if self._layout.gts is not None:
            with open(self._gts_path(color_path), "rb") as f:
                frame["gt_RTs"] = pickle.load(f)["gt_RTs"]      # one per object of interest, in the order of `objects`
        else:
            frame["depth"] = read_depth(depth_path)
            frame["coord"] = np.array(Image.open(self._frame_file(color_path, "coord.png")), dtype=np.uint8)
        return frame

    def _estimate_objects(self, frames: List[dict]) -> dict:
        """{(index into frames, mask id): (position, rotation, scale, transform) or None}: correspondences per frame,
        ONE fit launch for all objects of `frames`, one read-back."""
        dev = self._device
        sources, targets, owners, seeds, sizes = [], [], [], [], []
        for fi, frame in enumerate(frames):
            if not frame["objects"]:
                continue
            ids = [mask_id for mask_id, _ in frame["objects"]]
            c = nocs_utils.nocs_correspondences(torch.from_numpy(frame["depth"]).to(dev),
                                                torch.from_numpy(frame["mask"]).to(dev),
                                                torch.from_numpy(frame["coord"]).to(dev), ids, self._camera)
            sources.append(c.source)
            targets.append(c.target)
            for k, mask_id in enumerate(ids):
                # the reference's two rejections: too few correspondences, a depth that cannot be right
                ok = c.counts[k] >= nocs_utils.MIN_CORRESPONDENCES and not c.max_depth[k] > nocs_utils.MAX_DEPTH
                if c.max_depth[k] > nocs_utils.MAX_DEPTH:
                    print("Erroneous depth detected.")
                owners.append((fi, mask_id, ok))
                sizes.append(c.counts[k])
                seeds.append(((self._seed * 1000003 + frame["image_id"]) * 256 + mask_id) % (2 ** 63))
        estimates = {}
        if owners:
            offsets = np.concatenate([[0], np.cumsum(sizes)]).tolist()
            r = nocs_utils.estimate_similarity_transforms(
                torch.cat(sources), torch.cat(targets), offsets,
                object_seeds=torch.tensor(seeds, dtype=torch.int64, device=dev))
            status = r.status.cpu().tolist()
            pos, rot = r.position.cpu().numpy(), r.rotation_matrix.cpu().numpy()
            scale, T = r.scale.cpu().numpy(), r.transform.cpu().numpy()
            for k, (fi, mask_id, ok) in enumerate(owners):
                if ok and status[k] == nocs_utils.STATUS_NAN_INPUT:
                    raise RuntimeError("There are NANs in the input.")
                estimates[(fi, mask_id)] = (pos[k], rot[k], scale[k], T[k]) \
                    if ok and status[k] == nocs_utils.STATUS_OK else None
        return estimates

    def _annotate_frames(self, frames: List[dict], folder: str, stats: dict) -> list:
        """Writes the pickles of `frames` into `folder`; [(file name, category id)] of those written."""
        estimates = self._estimate_objects(frames) if self._layout.gts is None else {}
        written = []
        for fi, frame in enumerate(frames):
            kept = 0    # numbers the files of the frame, and, 0-based, the ground truth's poses
            for mask_id, meta_row in frame["objects"]:
                try:
                    if self._layout.gts is not None:
                        pose = pose_from_similarity_matrix(frame["gt_RTs"][kept]) + (frame["gt_RTs"][kept],)
                    else:
                        pose = estimates[(fi, mask_id)]
                    record = self._record(frame, mask_id, meta_row, pose)
                except PoseEstimationError:
                    print(f"Insufficient data for pose estimation. Skipping {frame['color_path']}:{mask_id}.")
                    stats["skipped"] += 1
                    continue
                except ObjectError:
                    print(f"Insufficient object mesh for pose estimation. Skipping {frame['color_path']}:{mask_id}.")
                    stats["skipped"] += 1
                    continue
                file_name = f"{frame['image_id']:08}_{kept}.pkl"
                with open(os.path.join(folder, file_name), "wb") as f:
                    pickle.dump(record, f)
                written.append((file_name, record["category_id"]))
                kept += 1
                stats["objects"] += 1
        return written

    def _record(self, frame: dict, mask_id: int, meta_row: list, pose: Optional[tuple]) -> dict:
        """What is stored for one object: paths, ids and, as float32 CPU tensors in the OpenCV camera frame, its
        position (3,), scalar-last quaternion (4,), bounding box side lengths (3,) and NOCS transform (4,4), with the
        box's diagonal and longest side.  pose: (position, rotation (3,3), NOCS scale, transform), or None where the
        fit failed (PoseEstimationError).  ObjectError for a mesh without vertices."""
        if pose is None:
            raise PoseEstimationError()
        position, rotation, nocs_scale, transform = pose
        obj_path = self._obj_path(meta_row)
        box = self._mesh_extents(obj_path)
        if self._layout.shapenet_models:    # unit-diagonal meshes: the NOCS scale IS the metric diagonal
            box = nocs_scale * box
        values = dict(nocs_transform=transform, position=position, orientation_q=matrix_to_quaternion(rotation),
                      extents=box)
        record = {"color_path": frame["color_path"], "depth_path": frame["depth_path"],
                  "mask_path": frame["mask_path"], "mask_id": mask_id, "category_id": meta_row[1], "obj_path": obj_path}
        for key in _RECORD_TENSORS:
            record[key] = torch.tensor(np.asarray(values[key]), dtype=torch.float32)
        record["nocs_scale"] = torch.linalg.norm(record["extents"])
        record["max_extent"] = torch.max(record["extents"])
        return record

    def _mesh_extents(self, obj_path: str) -> np.ndarray:
        from .mesh import Mesh
        vertices = Mesh.from_file(obj_path, device="cpu").vertices.numpy().astype(np.float64)
        if len(vertices) == 0:
            raise ObjectError()
        return vertices.max(axis=0) - vertices.min(axis=0)

    def _list_samples(self, folder: str, category_str: Optional[str] = None) -> list:
        """the folder's sample files in name order; of one category: the files categories.json lists for it"""
        if category_str is None:
            names = sorted(name for name in os.listdir(folder) if name.endswith(".pkl"))
        else:
            with open(os.path.join(folder, "categories.json")) as f:
                names = json.load(f)[category_str]
        return [os.path.join(folder, name) for name in names]

    # ---- samples ---------------------------------------------------------------------------------------------------
    def _sample_from_sample_data(self, sample_data: dict) -> dict:
        """The sample of a stored record (``__getitem__``): images and the point set on the device, the stored OpenCV
        pose in the configured object axes, camera convention, orientation representation and scale convention."""
        cfg, dev = self._config, self._device
        convention = cfg["camera_convention"]
        depth = torch.from_numpy(read_depth(sample_data["depth_path"])).to(dev)
        own_pixels = torch.from_numpy(read_instance_ids(sample_data["mask_path"])).to(dev) == sample_data["mask_id"]
        points = depth_to_pointcloud(depth, self._camera, mask=own_pixels if cfg["mask_pointcloud"] else None,
                                     convention=convention)
        quaternion, extents = self._in_object_axes(sample_data["orientation_q"], sample_data["extents"])
        quaternion = change_orientation_camera_convention(quaternion, "opencv", convention)
        position = change_position_camera_convention(sample_data["position"], "opencv", convention).to(dev)
        if cfg["normalize_pointcloud"]:
            points, centroid = normalize_points(points)
            position = position - centroid
        if self._orientation_grid is None:
            orientation = quaternion
        else:
            orientation = torch.tensor(self._orientation_grid.quat_to_index(quaternion.numpy()), dtype=torch.long)
        color = np.asarray(Image.open(sample_data["color_path"]), dtype=np.float32) / 255
        sample = {key: sample_data[key] for key in ("color_path", "obj_path", "category_id")}
        sample["category_str"] = self.category_id_to_str[sample_data["category_id"]]
        sample.update(color=torch.from_numpy(color).to(dev), depth=depth, mask=own_pixels, pointset=points,
                      position=position, orientation=orientation.to(dev), quaternion=quaternion.to(dev),
                      scale=torch.as_tensor(_SCALES[cfg["scale_convention"]](sample_data, extents)).to(dev))
        return sample

    def _in_object_axes(self, orientation_q: torch.Tensor, extents: torch.Tensor) -> tuple:
        """(quaternion, extents) for the remapped object axes; both unchanged without a remapping"""
        if self._object_axes is None:
            return orientation_q, extents
        axes = self._object_axes        # NOCS object frame -> new object frame
        new_extents = (torch.as_tensor(axes, dtype=extents.dtype) @ extents).abs()
        # stored: NOCS object -> camera; wanted: new object -> NOCS object -> camera
        back = torch.from_numpy(matrix_to_quaternion(axes.T))
        return quaternion_multiply(orientation_q, back), new_extents

    # ---- the trainer's validation batches ------------------------------------------------------------------------------
    def validation_batches(self, batch_size: int, max_points: int = 2500, seed: int = 0) -> list:
        """[(points (n, M, 3), targets)] for ``SDFPoseNetTrainer.validate``: consecutive samples in batches of
        `batch_size`, every point set reduced to M = min(the batch's smallest set, max_points) points drawn without
        replacement (the reference's ``dataset_utils.collate_samples``; the draws come from a host generator seeded
        with `seed`).  targets: "position", "scale", "orientation", "quaternion".  A NOCS sample has no latent."""
        gen = torch.Generator().manual_seed(int(seed))
        batches = []
        for first in range(0, len(self), batch_size):
            samples = [self[i] for i in range(first, min(first + batch_size, len(self)))]
            M = min(min(int(s["pointset"].shape[0]) for s in samples), int(max_points))
            if M < 1:
                raise ValueError("a sample without points cannot be collated")
            sets = [s["pointset"][torch.randperm(int(s["pointset"].shape[0]), generator=gen)[:M].to(self._device)]
                    for s in samples]
            targets = {k: torch.stack([s[k] for s in samples]) for k in ("position", "scale", "orientation", "quaternion")}
            batches.append((torch.stack(sets), targets))
        return batches
