"""CPU: ``sdfr_visible_mask`` is declared, bound, exported and validates its arguments before any HIP call;
``AnnotatedRedwoodDataset`` checks its config before any work, lists its samples as the reference does, and its
``annotation(idx)`` -- the pose half of a sample -- agrees with the float64 twin of the reference's lines
(tests/redwood_twin.py) for every scale convention, camera convention and axis remapping."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import redwood_scenes
import redwood_twin as twin
from helpers import ROOT

AXES = twin.AXES
VALID_PAIRS = [(x, y) for x, y in itertools.product(AXES, AXES) if x[-1] != y[-1]]
F32 = float(np.finfo(np.float32).eps)


def test_visible_mask_is_declared_bound_exported_and_validates_its_arguments():
    from sdfest_amd import _lib
    from test_cabi_symbols import declared_symbols
    assert "sdfr_visible_mask" in declared_symbols()
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES["sdfr_visible_mask"] == (i, [vp, vp, i, i, i, f, vp, vp, vp, i, vp])
    _lib.build()
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)   # a non-NULL pointer that is never dereferenced
    err = lambda: L.sdfr_last_error()
    call = lambda r, o, B, H, W, margin, m: L.sdfr_visible_mask(r, o, B, H, W, margin, m, None, None, 0, None)
    assert call(q, q, -1, 4, 4, 0.01, q) == -1 and b"B=-1" in err()
    assert call(q, q, 1, 0, 4, 0.01, q) == -1 and b"H=0" in err()
    assert call(q, q, 1, 4, 0, 0.01, q) == -1 and b"W=0" in err()
    assert call(q, q, 1, 4, 4, -0.01, q) == -1 and b"margin" in err()
    assert call(q, q, 1, 4, 4, float("nan"), q) == -1 and b"margin" in err()
    assert call(None, q, 1, 4, 4, 0.01, q) == -2 and b"NULL" in err()
    assert call(q, None, 1, 4, 4, 0.01, q) == -2
    assert call(q, q, 1, 4, 4, 0.01, None) == -2
    assert call(None, None, 0, 4, 4, 0.01, None) == 0      # nothing to do
    assert _lib.ABI["SDFR_E_INVALID"] == -1 and _lib.ABI["SDFR_E_NULL"] == -2
    # the Python front refuses what it can before the library is asked
    from sdfest_amd import visible_mask
    with pytest.raises(TypeError):
        visible_mask(torch.zeros(4, 4), torch.zeros(4, 4))
    with pytest.raises(ValueError):
        visible_mask(torch.zeros(4, 4), torch.zeros(4, 5))


# ---- the dataset's configuration ---------------------------------------------------------------------------------------
def dataset(folder, **config):
    from sdfest_amd import AnnotatedRedwoodDataset
    root_dir, ann_dir = redwood_scenes.write_annotations(folder)
    return AnnotatedRedwoodDataset(dict({"root_dir": root_dir, "ann_dir": ann_dir, "camera": redwood_scenes.CAMERA},
                                        **config))


def test_class_attributes_and_defaults_are_the_references():
    from sdfest_amd import AnnotatedRedwoodDataset as D
    assert D.num_categories == 3 and D.category_id_to_str == {0: "bottle", 1: "bowl", 2: "mug"}
    assert D.category_str_to_id == {"bottle": 0, "bowl": 1, "mug": 2}
    assert D.default_config == {"root_dir": None, "ann_dir": None, "mask_pointcloud": False,
                                "normalize_pointcloud": False, "camera_convention": "opengl",
                                "scale_convention": "half_max", "orientation_repr": "quaternion",
                                "orientation_grid_resolution": None, "category_str": None, "remap_y_axis": None,
                                "remap_x_axis": None}
    assert D.own_config["device"] == "cuda" and D.own_config["occlusion_margin"] == 0.01
    assert D.own_config["camera"] == dict(width=640, height=480, fx=525, fy=525, cx=319.5, cy=239.5)


@pytest.mark.parametrize("config, error", [
    ({"scale_convention": "radius"}, ValueError),
    ({"remap_x_axis": "z"}, ValueError),
    ({"remap_y_axis": "-y"}, ValueError),
    ({"remap_x_axis": "x", "remap_y_axis": "-x"}, ValueError),
    ({"orientation_repr": "euler"}, NotImplementedError),
    ({"category_str": "laptop"}, ValueError),
    ({"occlusion_margin": -1.0}, ValueError),
])
def test_config_errors_come_before_any_work(tmp_path, config, error):
    """no annotations.json exists below these folders: an error that came after the first file was read would be a
    FileNotFoundError"""
    from sdfest_amd import AnnotatedRedwoodDataset
    with pytest.raises(error):
        AnnotatedRedwoodDataset(dict({"root_dir": str(tmp_path / "r"), "ann_dir": str(tmp_path / "a")}, **config))


def test_missing_annotations_file(tmp_path):
    from sdfest_amd import AnnotatedRedwoodDataset
    with pytest.raises(FileNotFoundError):
        AnnotatedRedwoodDataset({"root_dir": str(tmp_path / "r"), "ann_dir": str(tmp_path / "a")})


def test_sample_order_and_category_filter(tmp_path):
    ds = dataset(tmp_path)
    assert len(ds) == 6
    anns = [ds.annotation(i) for i in range(6)]
    assert [a["category_str"] for a in anns] == ["mug"] * 3 + ["bottle"] * 3      # sequences in file order
    assert [a["category_id"] for a in anns] == [2] * 3 + [0] * 3
    root = os.path.join(str(tmp_path), "root")
    assert anns[1]["color_path"] == os.path.join(root, "mug", "rgbd", "seq_mug", "rgb", "0000001.jpg.png")
    assert anns[4]["depth_path"] == os.path.join(root, "bottle", "rgbd", "seq_box", "depth", "0000001.png")
    assert anns[4]["obj_path"] == os.path.join(str(tmp_path), "ann", "seq_box.obj")
    for i, a in enumerate(anns):        # pose_anns in order
        seq = "seq_mug" if i < 3 else "seq_box"
        assert np.allclose(a["position"].numpy() * [1, -1, -1], redwood_scenes.POSES[seq][i % 3][0], atol=1e-7)
    only = dataset(tmp_path, category_str="bottle")
    assert len(only) == 3 and all(only.annotation(i)["category_str"] == "bottle" for i in range(3))
    assert torch.equal(only.annotation(2)["position"], ds.annotation(5)["position"])
    assert len(dataset(tmp_path, category_str="bowl")) == 0


# ---- annotation(idx) against the twin ----------------------------------------------------------------------------------
def check_against_twin(ds, config):
    anns = __import__("json").load(open(os.path.join(ds._ann_dir, "annotations.json")))
    raw = [(p, seq) for seq in anns.values() for p in seq["pose_anns"]]
    for i, (pose, seq) in enumerate(raw):
        got = ds.annotation(i)
        want = twin.annotation(pose["position"], pose["orientation"], seq["scale"],
                               config.get("scale_convention", "half_max"), config.get("camera_convention", "opengl"),
                               config.get("remap_x_axis"), config.get("remap_y_axis"))
        # rotation matrices of the two quaternions (the sign is free): products of two float32 unit quaternions
        r_got = twin.quaternion_to_matrix(got["quaternion"].numpy().astype(np.float64))
        assert np.abs(r_got - twin.quaternion_to_matrix(want["quaternion"])).max() <= 1e-6, (i, config)
        assert abs(np.linalg.norm(got["quaternion"].numpy().astype(np.float64)) - 1) <= 1e-6
        # positions, extents and scales: float32 roundings of the annotated numbers (x 2 and the norm's few operations)
        assert np.abs(got["position"].numpy() - want["position"]).max() <= F32 * np.abs(want["position"]).max()
        assert np.abs(got["extents"].numpy() - want["extents"]).max() <= 2 * F32 * want["extents"].max()
        assert np.abs(got["scale"].numpy() - want["scale"]).max() <= 4 * F32 * np.max(want["scale"]), (i, config)
        assert tuple(got["scale"].shape) == ((3,) if config.get("scale_convention") == "full" else ())


@pytest.mark.parametrize("scale_convention", ["diagonal", "max", "half_max", "full"])
@pytest.mark.parametrize("camera_convention", ["opengl", "opencv"])
def test_annotation_conventions_against_the_twin(tmp_path, scale_convention, camera_convention):
    config = dict(scale_convention=scale_convention, camera_convention=camera_convention)
    check_against_twin(dataset(tmp_path, **config), config)
    config.update(remap_x_axis="z", remap_y_axis="-y")       # the ShapeNetV2 alignment
    check_against_twin(dataset(tmp_path, **config), config)


def test_annotation_all_valid_remaps_against_the_twin(tmp_path):
    assert len(VALID_PAIRS) == 24
    for camera_convention in ("opengl", "opencv"):
        for x, y in VALID_PAIRS:
            config = dict(remap_x_axis=x, remap_y_axis=y, camera_convention=camera_convention, scale_convention="full")
            check_against_twin(dataset(tmp_path, **config), config)


def test_parallel_remaps_raise_here_and_in_the_twin(tmp_path):
    pairs = [(x, y) for x, y in itertools.product(AXES, AXES) if x[-1] == y[-1]]
    assert len(pairs) == 12
    for x, y in pairs:
        with pytest.raises(ValueError):
            twin.o2n_matrix(x, y)
        with pytest.raises(ValueError):
            dataset(tmp_path, remap_x_axis=x, remap_y_axis=y)
    with pytest.raises(ValueError):
        dataset(tmp_path, remap_x_axis="up", remap_y_axis="y")


def test_twin_quaternion_round_trip():
    """the twin's own matrix -> quaternion (an eigenvector) against its quaternion -> matrix"""
    rng = np.random.default_rng(0)
    for _ in range(20):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        back = twin.matrix_to_quaternion(twin.quaternion_to_matrix(q))
        assert min(np.abs(back - q).max(), np.abs(back + q).max()) < 1e-12
    for x, y in VALID_PAIRS:
        m = twin.o2n_matrix(x, y)
        assert np.allclose(m @ m.T, np.eye(3)) and np.isclose(np.linalg.det(m), 1.0)
        assert np.array_equal(m[:, 2], np.cross(m[:, 0], m[:, 1]))


def test_known_answers_by_hand(tmp_path):
    pose = redwood_scenes.POSES["seq_box"][1]
    half = np.array(redwood_scenes.BOX_HALF)
    # the identity remap changes nothing
    plain, same = dataset(tmp_path).annotation(4), dataset(tmp_path, remap_x_axis="x", remap_y_axis="y").annotation(4)
    assert np.allclose(plain["quaternion"].numpy(), same["quaternion"].numpy(), atol=1e-7)
    assert torch.equal(plain["extents"], same["extents"])
    # opencv: the annotated numbers; opengl: (x, -y, -z)
    cv = dataset(tmp_path, camera_convention="opencv").annotation(4)
    assert np.array_equal(cv["position"].numpy(), np.float32(pose[0]))
    assert np.array_equal(cv["quaternion"].numpy(), np.float32(pose[1]))
    assert np.array_equal(plain["position"].numpy(), np.float32(pose[0]) * np.float32([1, -1, -1]))
    # extents: twice the annotated half sides; under ("z", "-y") |R e| = (e_z, e_y, e_x)
    assert np.array_equal(plain["extents"].numpy(), np.float32(half) * 2)
    remapped = dataset(tmp_path, remap_x_axis="z", remap_y_axis="-y").annotation(4)
    R = np.array([[0, 0, 1.0], [0, -1, 0], [1, 0, 0]])        # columns: x -> z, y -> -y, z -> x
    assert np.array_equal(remapped["extents"].numpy(), np.abs(R @ (np.float32(half) * 2).astype(np.float64)).astype(np.float32))
    assert np.array_equal(remapped["extents"].numpy(), (np.float32(half) * 2)[[2, 1, 0]])
    # the scale conventions of a known box
    e = np.float32(half) * 2
    for name, want in (("diagonal", np.linalg.norm(e)), ("max", e.max()), ("half_max", 0.5 * e.max())):
        assert dataset(tmp_path, scale_convention=name).annotation(4)["scale"].item() == pytest.approx(want, rel=1e-6)


def test_discretized_orientation_is_the_grids_cell(tmp_path):
    from sdfest_amd import SO3Grid
    for camera_convention in ("opengl", "opencv"):
        ds = dataset(tmp_path, orientation_repr="discretized", orientation_grid_resolution=1,
                     camera_convention=camera_convention, remap_x_axis="z", remap_y_axis="-y")
        grid = SO3Grid(1)
        for i in range(len(ds)):
            a = ds.annotation(i)
            assert a["orientation"].dtype == torch.int64 and a["orientation"].dim() == 0
            assert a["orientation"].item() == grid.quat_to_index(a["quaternion"].numpy())
            assert a["quaternion"].shape == (4,)
    quat = dataset(tmp_path).annotation(0)
    assert torch.equal(quat["orientation"], quat["quaternion"])


def test_evaluation_refuses_normalised_samples_before_any_work(tmp_path):
    from sdfest_amd.evaluation import evaluate_annotated
    ds = dataset(tmp_path, normalize_pointcloud=True)
    with pytest.raises(ValueError, match="normalize_pointcloud"):
        evaluate_annotated(object(), ds, 100, 0)
    with pytest.raises(ValueError, match="frames_per_call"):
        evaluate_annotated(object(), dataset(tmp_path), 100, 0, frames_per_call=0)


def test_pose_errors_by_hand():
    from sdfest_amd.evaluation import DEFAULT_POSE_THRESHOLDS, pose_errors
    assert DEFAULT_POSE_THRESHOLDS == {"5deg_2cm": (5.0, 0.02), "5deg_5cm": (5.0, 0.05), "10deg_2cm": (10.0, 0.02),
                                       "10deg_5cm": (10.0, 0.05)}
    half = np.deg2rad(30.0) / 2
    about_z = [0.0, 0.0, np.sin(half), np.cos(half)]
    p, r = pose_errors([0, 0, 0.5], [0, 0, 0, 1.0], [0.03, 0, 0.54], about_z)
    assert p == pytest.approx(0.05, abs=1e-12) and r == pytest.approx(30.0, abs=1e-9)
    assert pose_errors([0, 0, 0.5], [0, 0, 0, 1.0], [0, 0, 0.5], about_z, 2)[1] == pytest.approx(0.0, abs=1e-6)
    assert pose_errors([0, 0, 0.5], [0, 0, 0, 1.0], [0, 0, 0.5], about_z, 0)[1] == pytest.approx(30.0, abs=1e-9)


def test_tool_help_exits_0():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "redwood_evaluation.py"), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "category_configs" in res.stdout
