"""CPU: tests/nocs_twin.py's RANSAC half against the reference's recorded runs (tests/golden/nocs_ransac.npz, captured
by tools/make_nocs_goldens.py with the reference's own draws).  Choices equal exactly; outputs to 1e-10, the bound of
the reference's own test_nocs_utils.py."""
import ctypes
import os

import numpy as np
import pytest

import nocs_twin as tw
from helpers import GOLDEN

ATOL = 1e-10


def load_cases():
    d = np.load(os.path.join(GOLDEN, "nocs_ransac.npz"))
    cases = {}
    for name in d["cases"]:
        prefix = f"{name}."
        cases[str(name)] = {k[len(prefix):]: d[k] for k in d.files if k.startswith(prefix)}
    return cases


CASES = load_cases()


def test_golden_cases_are_the_ones_the_tests_rely_on():
    assert sorted(CASES) == ["a", "b4", "b5", "c", "d", "e", "f", "g0", "g1", "g2", "g3", "g4"]
    assert int(CASES["a"]["iterations_run"]) == 1 and len(CASES["a"]["source"]) == 10
    assert len(CASES["b5"]["source"]) == 5 and int(CASES["b5"]["status"]) == tw.OK
    assert len(CASES["b4"]["source"]) == 4 and int(CASES["b4"]["status"]) == tw.NONE
    c = CASES["c"]
    assert len(c["source"]) == 257 and int(c["iterations_run"]) == 100 and c["source"].dtype == np.float32
    d = CASES["d"]
    assert 3 <= int(d["iterations_run"]) - 1 <= 60 and int(d["best_iteration"]) == int(d["iterations_run"]) - 1
    assert int(d["no_stop_winner"]) != int(d["best_iteration"])      # the early stop decides the winner
    assert int(CASES["e"]["status"]) == tw.NONE and float(CASES["e"]["inlier_ratio"]) < 0.1
    assert int(CASES["f"]["status"]) == tw.POSE_ERROR
    for g in range(5):
        c = CASES[f"g{g}"]
        assert c["source"].dtype == np.float32 and 3000 < len(c["source"]) < 5100 and int(c["status"]) == tw.OK


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_replays_the_reference(name):
    c = CASES[name]
    o = tw.ransac(c["source"], c["target"], c["draws"])
    assert o["status"] == int(c["status"])
    assert o["iterations_run"] == int(c["iterations_run"])
    if o["status"] == tw.POSE_ERROR:
        return
    assert o["best_iteration"] == int(c["best_iteration"])
    assert np.array_equal(o["inlier_idx"], c["inlier_idx"])
    assert o["inlier_ratio"] == float(c["inlier_ratio"])
    if "residuals" in c:
        np.testing.assert_allclose(o["residuals"], c["residuals"], rtol=1e-12)
    if o["status"] == tw.OK:
        for key in ("position", "rotation", "scale", "transform"):
            np.testing.assert_allclose(o[key], c[key], rtol=0, atol=ATOL)


def test_twin_return_convention():
    c = CASES["c"]
    pos, rot, scale, T = tw.estimate_similarity_transform(c["source"], c["target"], c["draws"])
    np.testing.assert_allclose(T[:3, :3], scale * rot, atol=1e-14)
    np.testing.assert_allclose(T[:3, 3], pos, atol=0)
    assert tw.estimate_similarity_transform(CASES["e"]["source"], CASES["e"]["target"], CASES["e"]["draws"]) == (None,) * 4
    assert tw.estimate_similarity_transform(CASES["b4"]["source"], CASES["b4"]["target"], CASES["b4"]["draws"]) == (None,) * 4
    with pytest.raises(tw.PoseEstimationError):
        tw.estimate_similarity_transform(CASES["f"]["source"], CASES["f"]["target"], CASES["f"]["draws"])


def test_inlier_ratio_never_counts_point_zero():
    """the reference's quirk: count_nonzero of the inlier INDICES"""
    c = CASES["a"]
    assert 0 in c["inlier_idx"] and len(c["inlier_idx"]) == 10 and float(c["inlier_ratio"]) == 0.9


def test_frame_fixture_gives_the_golden_correspondences():
    f = np.load(os.path.join(GOLDEN, "nocs_frame.npz"))
    depth = f["depth_mm"].astype(np.float32) * np.float32(0.001)
    for g, mid in enumerate(f["meta_mask_id"]):
        s, t, zmax = tw.correspondences(depth, f["mask"], f["coord"], int(mid))
        assert np.array_equal(s, CASES[f"g{g}"]["source"]) and np.array_equal(t, CASES[f"g{g}"]["target"])
        assert 0 < zmax < 32


def test_nocs_entry_points_validate_their_arguments_without_gpu():
    from sdfest_amd import _lib
    _lib.build()
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)   # a non-NULL pointer that is never dereferenced
    err = lambda: L.sdfr_last_error()
    assert _lib.ABI["SDFR_NOCS_HYPOTHESES"] == 100
    assert L.sdfr_nocs_workspace_bytes(640, 480, 5) == 5 * 300 * 8 and L.sdfr_nocs_workspace_bytes(0, 480, 5) == 0
    assert L.sdfr_nocs_count(q, q, 640, 480, q, -1, q, q, q, 1 << 20, 0, None) == -1 and b"K=-1" in err()
    assert L.sdfr_nocs_count(q, None, 640, 480, q, 2, q, q, q, 1 << 20, 0, None) == -2
    assert L.sdfr_nocs_count(q, q, 640, 480, q, 2, q, q, q, 16, 0, None) == -3 and b"workspace" in err()
    assert L.sdfr_nocs_count(None, None, 640, 480, None, 0, None, None, None, 0, 0, None) == 0
    assert L.sdfr_nocs_correspondences(q, q, q, 2, 640, 480, 1.0, 1.0, 0.0, 0.0, q, 1, q, 10, q, q, q, 0, None) == -1
    assert b"channels" in err()
    assert L.sdfr_nocs_correspondences(q, q, q, 3, 640, 480, 1.0, 1.0, 0.0, 0.0, q, 1, q, -1, q, q, q, 0, None) == -1
    assert L.sdfr_nocs_correspondences(q, q, q, 3, 640, 480, 1.0, 1.0, 0.0, 0.0, q, 1, None, 10, q, q, q, 0, None) == -2
    ransac = lambda **kw: L.sdfr_similarity_ransac(kw.get("src", q), q, kw.get("dtype", 0), kw.get("off", q),
                                                   kw.get("total", 100), kw.get("max_n", 50), kw.get("K", 2), q, q, q,
                                                   q, q, q, q, q, kw.get("status", q), None, q, kw.get("wsn", 1 << 30),
                                                   0, None)
    assert ransac(K=0) == -1 and ransac(total=-1) == -1 and ransac(max_n=-1) == -1
    assert ransac(max_n=101) == -1 and b"max_n" in err()
    assert ransac(dtype=2) == -1 and b"dtype" in err()
    assert ransac(src=None) == -2 and ransac(off=None) == -2 and ransac(status=None) == -2
    assert ransac(wsn=64) == -3 and b"workspace" in err()
    assert L.sdfr_similarity_ransac_workspace_bytes(0, 10, 10) == 0
    assert L.sdfr_similarity_ransac_workspace_bytes(2, 100, 50) % 128 == 0
    assert L.sdfr_nocs_sample_indices(q, -1, 0, None, q, 0, None) == -1
    assert L.sdfr_nocs_sample_indices(None, 2, 0, None, q, 0, None) == -2
    assert L.sdfr_nocs_sample_indices(None, 0, 0, None, None, 0, None) == 0
    assert _lib.ABI["SDFR_NOCS_TRUNCATED"] == 4


AXES = ["x", "-x", "y", "-y", "z", "-z"]


def test_object_axes_matrix_equals_the_twin():
    """every pair of axis names: the 24 non-parallel ones give the twin's matrix (built another way: the third column
    from the row sums and the determinant), the 12 parallel ones and unknown names a ValueError"""
    from sdfest_amd.nocs_dataset import object_axes_matrix
    valid = 0
    for to_x in AXES:
        for to_y in AXES:
            if to_x[-1] == to_y[-1]:
                with pytest.raises(ValueError):
                    object_axes_matrix(to_x, to_y)
                continue
            r = object_axes_matrix(to_x, to_y)
            assert r.tobytes() == (tw.remap_matrix(to_y, to_x) + 0.0).tobytes(), (to_x, to_y)
            assert np.linalg.det(r) == 1.0 and np.array_equal(r @ r.T, np.eye(3))
            valid += 1
    assert valid == 24
    for bad in [("w", "y"), ("x", "+y"), ("x", None)]:
        with pytest.raises(ValueError):
            object_axes_matrix(*bad)


def test_pose_from_similarity_matrix():
    from sdfest_amd.nocs_dataset import pose_from_similarity_matrix
    rot = tw.umeyama(CASES["a"]["source"][:5], CASES["a"]["target"][:5])[1]
    T = np.eye(4)
    T[:3, :3] = 0.37 * rot
    T[:3, 3] = [0.1, -0.2, 0.9]
    position, rotation, scale = pose_from_similarity_matrix(T)
    assert np.array_equal(position, T[:3, 3]) and abs(scale - 0.37) < 1e-15
    np.testing.assert_allclose(rotation, rot, rtol=0, atol=1e-15)


def test_dataset_checks_its_config_before_any_work(tmp_path):
    """a config that no sample could be made from fails at construction, with nothing written"""
    from sdfest_amd import NOCSDataset
    base = {"root_dir": str(tmp_path), "split": "real_train", "device": "cpu"}
    for bad, error in ((dict(split="real"), ValueError), (dict(scale_convention="min"), ValueError),
                       (dict(category_str="cup"), ValueError), (dict(remap_y_axis="y"), ValueError),
                       (dict(remap_y_axis="y", remap_x_axis="-y"), ValueError),
                       (dict(orientation_repr="euler"), NotImplementedError)):
        with pytest.raises(error):
            NOCSDataset({**base, **bad})
    assert os.listdir(tmp_path) == []
