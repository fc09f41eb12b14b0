"""GPU: the 3D IoU in ``evaluation.evaluate_annotated`` (``iou_thresholds``) on the small annotated set of
tests/redwood_scenes.py, with a stand-in pipeline that answers the annotation itself -- exactly, shifted by a known
vector, or spun about a symmetry axis -- against the numpy twin (tests/box_iou_twin.py) on the same two boxes."""
import numpy as np
import pytest
import torch

import box_iou_twin as twin
import redwood_scenes

pytestmark = pytest.mark.gpu

SAMPLES = 500
NAMES = ["5deg_2cm", "5deg_5cm", "10deg_2cm", "10deg_5cm"]
THRESHOLDS = {"iou25": 0.25, "iou50": 0.5, "iou90": 0.9}


@pytest.fixture(scope="module")
def ds(tmp_path_factory):
    from sdfest_amd import AnnotatedRedwoodDataset
    scene = redwood_scenes.write_scene(tmp_path_factory.mktemp("redwood_iou"))
    return AnnotatedRedwoodDataset({"root_dir": scene["root_dir"], "ann_dir": scene["ann_dir"], "camera": scene["camera"],
                                    "camera_convention": "opencv"})


def y_turn(degrees):
    half = np.deg2rad(degrees) / 2
    return torch.tensor(np.round([0.0, np.sin(half), 0.0, np.cos(half)], 15), dtype=torch.float64)   # 180: (0, 1, 0, 0)


class Annotation:
    """a pipeline that answers a frame with its own annotation in the OpenGL frame (found by the depth image), moved by
    `shift` (3,) and spun about the object's own axes by the quaternion `spin`, in float64 (a pipeline may return any
    float dtype); generate_mesh returns the ground-truth mesh of the sample the "latent" names"""

    def __init__(self, ds, shift=None, spin=None):
        from sdfest_amd.pipeline import quaternion_multiply
        from sdfest_amd.pointset_utils import change_orientation_camera_convention, change_position_camera_convention
        self.ds = ds
        self.samples = ds.samples(range(len(ds)))
        self.poses = []
        for s in self.samples:
            p = change_position_camera_convention(s["position"], "opencv", "opengl").double()
            q = change_orientation_camera_convention(s["quaternion"], "opencv", "opengl").double()
            if shift is not None:
                p = p + torch.as_tensor(shift, dtype=torch.float64, device=p.device)
            if spin is not None:
                q = quaternion_multiply(q, spin.to(q.device))
            self.poses.append((p[None], q[None]))

    def __call__(self, depth, mask, color, shape_optimization=True):
        index = next(i for i, s in enumerate(self.samples) if torch.equal(s["depth"], depth))
        p, q = self.poses[index]
        return p, q, torch.ones(1, device="cuda"), torch.tensor([[float(index)]], device="cuda")

    def generate_mesh(self, latent, scale, complete_mesh=False):
        return self.ds.load_mesh(self.samples[int(latent.reshape(-1)[0].item())]["obj_path"])


def expected(ds, pipe, index, symmetry_axis=None):
    """(IoU by the twin, its bound, the two boxes) of sample `index`: the annotated box against the loaded mesh's posed
    tight box -- the box ``Mesh.oriented_box`` returns for the stand-in's float64 pose, so that twin and kernel read the
    same numbers"""
    from sdfest_amd.pointset_utils import change_orientation_camera_convention, change_position_camera_convention
    s = pipe.samples[index]
    host = lambda t: t.detach().double().cpu().numpy()
    gt = (host(change_position_camera_convention(s["position"], "opencv", "opengl")),
          host(change_orientation_camera_convention(s["quaternion"], "opencv", "opengl")), host(ds.annotation(index)["extents"]))
    mesh = ds.load_mesh(s["obj_path"])
    position, orientation = pipe.poses[index][0][0], pipe.poses[index][1][0]
    box = tuple(host(t) for t in mesh.oriented_box(position, orientation))
    # the tight box itself, in float64 from the same float32 vertices
    c, _, e = twin.tight_box(host(mesh.scaled_vertices()), host(position), host(orientation))
    assert np.allclose(box[0], c, rtol=0, atol=1e-12) and np.allclose(box[2], e, rtol=0, atol=1e-12)
    V, iou = twin.box_intersection(gt, box, symmetry_axis, 20)
    L = twin.length_scale(gt[0], gt[2], box[0], box[2])
    return iou, 2e-12 * L ** 3 / (np.prod(gt[2]) + np.prod(box[2]) - V), gt, box


def test_without_thresholds_nothing_changes_and_with_them_the_iou_is_the_twins(ds):
    from sdfest_amd.evaluation import DEFAULT_METRICS, evaluate_annotated
    pipe = Annotation(ds)
    plain = evaluate_annotated(pipe, ds, SAMPLES, 0)
    assert sorted(plain) == ["correct", "samples", "skipped", "stats"] and sorted(plain["correct"]) == sorted(NAMES)
    for e in plain["samples"]:
        assert sorted(e) == ["category_str", "correct", "index", "metrics", "position_error", "rotation_error"]
        assert sorted(e["correct"]) == sorted(NAMES)
    assert sorted(plain["stats"]["all"]) == sorted(list(DEFAULT_METRICS) + ["position_error", "rotation_error"])

    result = evaluate_annotated(pipe, ds, SAMPLES, 0, iou_thresholds=THRESHOLDS)
    assert [e["index"] for e in result["samples"]] == list(range(6))
    for e, before in zip(result["samples"], plain["samples"]):
        want, bound, gt, box = expected(ds, pipe, e["index"])
        print(f"sample {e['index']} ({e['category_str']}): IoU {e['iou_3d']!r}, twin {want!r}")
        assert abs(e["iou_3d"] - want) <= bound
        assert e["correct"] == dict(before["correct"], **{n: int(e["iou_3d"] >= t) for n, t in THRESHOLDS.items()})
        assert {k: v for k, v in e.items() if k not in ("iou_3d", "correct")} == {k: v for k, v in before.items()
                                                                                 if k != "correct"}
        if e["category_str"] == "bottle":      # the box mesh is its own annotated box, to float32 accuracy: a centre
            assert e["iou_3d"] >= 1.0 - 1e-4   # good to 6e-8 m on sides of 0.07 m costs about 1e-6 per axis
    values = [e["iou_3d"] for e in result["samples"]]
    for name, t in THRESHOLDS.items():
        assert result["correct"][name] == sum(v >= t for v in values) / 6
    assert {n: result["correct"][n] for n in NAMES} == plain["correct"]
    assert result["stats"]["all"]["iou_3d"]["mean"] == pytest.approx(sum(values) / 6, abs=1e-15)
    assert sorted(result["stats"]["bottle"]) == sorted(list(DEFAULT_METRICS) + ["iou_3d", "position_error",
                                                                                "rotation_error"])


def test_a_known_shift_lowers_the_iou_to_the_twins_value(ds):
    from sdfest_amd.evaluation import evaluate_annotated
    exact = Annotation(ds)
    moved = Annotation(ds, shift=[0.02, -0.01, 0.015])
    result = evaluate_annotated(moved, ds, SAMPLES, 0, iou_thresholds={"iou50": 0.5}, indices=[1, 3, 4])
    for e in result["samples"]:
        want, bound, _, _ = expected(ds, moved, e["index"])
        unmoved, _, _, _ = expected(ds, exact, e["index"])
        assert abs(e["iou_3d"] - want) <= bound and e["iou_3d"] < unmoved - 0.05
        assert e["correct"]["iou50"] == int(e["iou_3d"] >= 0.5)


def test_a_spin_about_the_symmetry_axis_keeps_the_iou(ds):
    """The box (sides 0.1, 0.07, 0.16) spun about its own y axis by two of the twenty steps (36 degrees) and by ten (a
    half turn): with the category's symmetry axis the IoU stays at the unspun value within 1e-9 and is the twin's on the
    same two boxes; without the axis the 36-degree spin is seen."""
    from sdfest_amd.evaluation import evaluate_annotated
    bottles = [3, 4, 5]
    run = lambda pipe, **kw: evaluate_annotated(pipe, ds, SAMPLES, 0, iou_thresholds=THRESHOLDS, indices=bottles,
                                                **kw)["samples"]
    unspun = run(Annotation(ds), symmetry_axes={"bottle": 1})
    for degrees in (36.0, 180.0):
        spun_pipe = Annotation(ds, spin=y_turn(degrees))
        for a, b in zip(unspun, run(spun_pipe, symmetry_axes={"bottle": 1})):
            want, bound, _, _ = expected(ds, spun_pipe, b["index"], symmetry_axis=1)
            print(f"sample {a['index']}: IoU {a['iou_3d']!r}, spun by {degrees:g} degrees {b['iou_3d']!r} (twin {want!r})")
            assert abs(b["iou_3d"] - a["iou_3d"]) <= 1e-9
            assert abs(b["iou_3d"] - want) <= bound
            assert b["correct"] == a["correct"]
    for c in run(Annotation(ds, spin=y_turn(36.0))):
        print(f"sample {c['index']}: spun by 36 degrees, without the axis {c['iou_3d']!r}")
        assert c["iou_3d"] < 0.8 and c["correct"]["iou90"] == 0
