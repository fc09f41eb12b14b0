"""GPU: ``AnnotatedRedwoodDataset`` samples on the small annotated set of tests/redwood_scenes.py -- the mask against
the torch expression on ``draw_depth_geometry`` of the loaded mesh, the three patches (an occluder, a reading within
the margin, no reading), the point set, normalisation, ``samples`` against ``__getitem__`` bit for bit, ``load_mesh``
under a remapping, and ``validation_batches`` through ``SDFPoseNetTrainer.validate``."""
import numpy as np
import pytest
import torch
from PIL import Image

import redwood_scenes

pytestmark = pytest.mark.gpu

KEYS = ["category_id", "category_str", "color", "color_path", "depth", "mask", "obj_path", "orientation", "pointset",
        "position", "quaternion", "scale"]


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return redwood_scenes.write_scene(tmp_path_factory.mktemp("redwood"))


def dataset(scene, **config):
    from sdfest_amd import AnnotatedRedwoodDataset
    return AnnotatedRedwoodDataset(dict({"root_dir": scene["root_dir"], "ann_dir": scene["ann_dir"],
                                         "camera": scene["camera"]}, **config))


def test_sample_keys_mask_and_patches(scene):
    from sdfest_amd import Mesh, draw_depth_geometry
    ds = dataset(scene)
    assert len(ds) == 6
    for i in range(6):
        s = ds[i]
        assert sorted(s) == KEYS
        assert all(s[k].is_cuda for k in ("color", "depth", "mask", "pointset", "position", "orientation", "quaternion",
                                          "scale"))
        assert tuple(s["depth"].shape) == (120, 160) and s["depth"].dtype == torch.float32
        assert tuple(s["color"].shape) == (120, 160, 3) and s["mask"].dtype == torch.bool
        # the files as the reference reads them
        depth = torch.from_numpy(np.asarray(Image.open(ds.annotation(i)["depth_path"]), dtype=np.float32) * 0.001).cuda()
        assert torch.equal(s["depth"], depth)
        color = np.asarray(Image.open(s["color_path"]), dtype=np.float32) / 255
        assert np.array_equal(s["color"].cpu().numpy(), color)
        # _compute_mask: the mesh as it is in its file, at the raw annotated (OpenCV) pose
        seq = "seq_mug" if i < 3 else "seq_box"
        mesh = Mesh.from_file(s["obj_path"], 1.0, rel_scale=True, center=False)
        mesh.position, mesh.orientation = redwood_scenes.POSES[seq][i % 3]
        r = draw_depth_geometry(mesh, ds.camera)
        want = (r != 0) & ~((depth != 0) & (depth < r - 0.01))
        assert torch.equal(s["mask"], want)
        covered = (r != 0).cpu().numpy()
        mask = s["mask"].cpu().numpy()
        patches = scene["patches"][i]
        assert all(p.sum() >= redwood_scenes.MIN_PATCH and covered[p].all() for p in patches.values())
        assert not mask[patches["occluded"]].any()          # 5 cm in front of the object
        assert mask[patches["near"]].all()                   # 5 mm in front: within the margin
        assert mask[patches["zero"]].all()                   # no reading: still the object's pixel
        assert not mask[~covered].any()
        assert mask[covered & ~patches["occluded"]].all()
        assert not s["depth"].cpu().numpy()[patches["zero"]].any()


@pytest.mark.parametrize("convention", ["opengl", "opencv"])
def test_pointset_with_and_without_the_mask(scene, convention):
    from sdfest_amd import Mesh, draw_depth_geometry, visible_mask
    from sdfest_amd.pointset_utils import depth_to_pointcloud
    plain = dataset(scene, camera_convention=convention)
    masked = dataset(scene, camera_convention=convention, mask_pointcloud=True)
    for i in (1, 4):
        a, b = plain[i], masked[i]
        assert torch.equal(a["mask"], b["mask"]) and torch.equal(a["depth"], b["depth"])
        assert torch.equal(a["pointset"], depth_to_pointcloud(a["depth"], plain.camera, convention=convention))
        assert torch.equal(b["pointset"], depth_to_pointcloud(b["depth"], plain.camera, mask=b["mask"],
                                                              convention=convention))
        assert a["pointset"].shape[0] == int((a["depth"] != 0).sum())
        # the masked set's length is the kernel's `valid` count: visible pixels with a reading (none from the zero patch)
        valid = int((b["mask"] & (b["depth"] != 0)).sum())
        assert b["pointset"].shape[0] == valid == int(b["mask"].sum()) - int(scene["patches"][i]["zero"].sum())
        mesh = Mesh.from_file(b["obj_path"], 1.0, rel_scale=True, center=False)
        mesh.position, mesh.orientation = redwood_scenes.POSES["seq_mug" if i < 3 else "seq_box"][i % 3]
        counts = visible_mask(draw_depth_geometry(mesh, plain.camera), b["depth"], 0.01, return_counts=True)[1].tolist()
        assert counts[3] == valid and counts[1] == int(b["mask"].sum()) and counts[0] == counts[1] + counts[2]
        assert counts[2] == int(scene["patches"][i]["occluded"].sum())
        sign = 1.0 if convention == "opencv" else -1.0
        assert (sign * b["pointset"][:, 2] > 0).all()
        assert torch.equal(a["position"], plain.annotation(i)["position"].cuda())


def test_normalised_samples(scene):
    from sdfest_amd.pointset_utils import normalize_points
    for mask_pointcloud in (False, True):
        plain = dataset(scene, mask_pointcloud=mask_pointcloud)
        normalised = dataset(scene, mask_pointcloud=mask_pointcloud, normalize_pointcloud=True)
        for i in (0, 5):
            a, b = plain[i], normalised[i]
            points, centroid = normalize_points(a["pointset"])
            assert torch.equal(b["pointset"], points)
            assert torch.equal(b["position"], a["position"] - centroid)       # the same centroid, bit for bit
            assert b["pointset"].mean(0).abs().max().item() < 1e-6
            assert torch.equal(a["quaternion"], b["quaternion"]) and torch.equal(a["scale"], b["scale"])


def test_samples_equal_getitem_bit_for_bit(scene):
    ds = dataset(scene, mask_pointcloud=True, remap_x_axis="z", remap_y_axis="-y", scale_convention="full")
    together = ds.samples(range(6))
    assert len(together) == 6 and ds.samples([]) == []
    for i in range(6):
        one = ds[i]
        assert sorted(one) == sorted(together[i]) == KEYS
        for k in KEYS:
            if isinstance(one[k], torch.Tensor):
                assert torch.equal(one[k], together[i][k]), (i, k)
            else:
                assert one[k] == together[i][k], (i, k)
    # any order, a sample twice, the two meshes interleaved
    mixed = ds.samples([4, 0, 4, 2])
    for got, i in zip(mixed, [4, 0, 4, 2]):
        assert torch.equal(got["mask"], together[i]["mask"]) and torch.equal(got["pointset"], together[i]["pointset"])
    assert len(ds._meshes) == 2                              # one mesh per sequence, read once


def test_load_mesh_under_a_remap(scene):
    from sdfest_amd import Mesh
    from sdfest_amd.nocs_dataset import object_axes_matrix
    path = dataset(scene).annotation(0)["obj_path"]
    raw = Mesh.from_file(path, 1.0, rel_scale=True)
    same = dataset(scene).load_mesh(path)
    assert torch.equal(same.vertices, raw.vertices) and torch.equal(same.faces, raw.faces)
    ds = dataset(scene, remap_x_axis="z", remap_y_axis="-y")
    turned = ds.load_mesh(path)
    R = torch.tensor(object_axes_matrix("z", "-y"), dtype=torch.float32, device="cuda")
    assert torch.equal(turned.vertices, (R @ raw.vertices.T).T) and torch.equal(turned.faces, raw.faces)
    assert torch.equal(turned.vertices, raw.vertices[:, [2, 1, 0]] * torch.tensor([1.0, -1.0, 1.0], device="cuda"))
    assert not turned.position.any() and turned.orientation.tolist() == [0.0, 0.0, 0.0, 1.0]
    # the remapped mesh under the remapped quaternion is the annotated mesh under the annotated one
    a0, a1 = dataset(scene, camera_convention="opencv").annotation(0), dataset(
        scene, camera_convention="opencv", remap_x_axis="z", remap_y_axis="-y").annotation(0)
    raw.orientation, turned.orientation = a0["quaternion"], a1["quaternion"]
    assert (raw.transformed_vertices() - turned.transformed_vertices()).abs().max().item() < 1e-6


def test_validation_batches_run_through_the_trainer(scene):
    import init_train_twin as it
    from sdfest_amd import SDFPoseNetTrainer
    from sdfest_amd.init_train import validation_keys
    ds = dataset(scene, mask_pointcloud=True, normalize_pointcloud=True, orientation_repr="discretized",
                 orientation_grid_resolution=it.P16["orientation_grid_resolution"])
    batches = ds.validation_batches(4, max_points=100, seed=3)
    assert [b[0].shape[0] for b in batches] == [4, 2]
    for points, targets in batches:
        assert points.is_cuda and points.shape[1:] == (100, 3)
        assert sorted(targets) == ["orientation", "position", "quaternion", "scale"]
        assert targets["orientation"].dtype == torch.int64 and targets["quaternion"].dtype == torch.float32
    again = ds.validation_batches(4, max_points=100, seed=3)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(batches, again))
    trainer = SDFPoseNetTrainer(it.train_config(it.P16), seed=4)
    got = trainer.validate(batches, "redwood")
    assert list(got) == validation_keys("redwood", True)
    assert all(np.isfinite(v) for v in got.values())
