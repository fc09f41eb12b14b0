"""GPU: ``evaluation.evaluate_annotated`` on the small annotated set of tests/redwood_scenes.py -- with a stand-in
pipeline that answers the annotation itself (exactly, offset by a known amount, turned about a symmetry axis), and with
the real ``SDFPipeline`` against the same steps composed by hand from the public functions."""
import json

import numpy as np
import pytest
import torch

import redwood_scenes

pytestmark = pytest.mark.gpu

SAMPLES = 2000
NAMES = ["5deg_2cm", "5deg_5cm", "10deg_2cm", "10deg_5cm"]


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return redwood_scenes.write_scene(tmp_path_factory.mktemp("redwood_eval"))


def dataset(scene, **config):
    from sdfest_amd import AnnotatedRedwoodDataset
    return AnnotatedRedwoodDataset(dict({"root_dir": scene["root_dir"], "ann_dir": scene["ann_dir"],
                                         "camera": scene["camera"]}, **config))


def qmul(a, b):
    from sdfest_amd.pipeline import quaternion_multiply
    return quaternion_multiply(a, b)


def axis_angle(axis, degrees):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    half = np.deg2rad(degrees) / 2
    return torch.tensor(np.append(np.sin(half) * axis, np.cos(half)), dtype=torch.float64)


class StandIn:
    """answers a frame with its own annotation, in the pipeline's OpenGL frame: found by the depth image it is given;
    the "latent" is the sample's index, from which generate_mesh returns the ground-truth mesh.  shift (3,): added to
    the position; turn: a quaternion applied in the camera frame; spin: one applied in the object frame."""

    def __init__(self, ds, shift=None, turn=None, spin=None):
        from sdfest_amd.pointset_utils import change_orientation_camera_convention, change_position_camera_convention
        self.ds, self.frames_calls = ds, 0
        convention = ds._config["camera_convention"]
        self.samples = ds.samples(range(len(ds)))
        self.poses = []
        for s in self.samples:
            p = change_position_camera_convention(s["position"], convention, "opengl").double()
            q = change_orientation_camera_convention(s["quaternion"], convention, "opengl").double()
            if shift is not None:
                p = p + torch.as_tensor(shift, dtype=torch.float64, device=p.device)
            if turn is not None:
                q = qmul(turn.to(q.device), q)
            if spin is not None:
                q = qmul(q, spin.to(q.device))
            self.poses.append((p.float()[None], q.float()[None]))

    def _answer(self, depth):
        index = next(i for i, s in enumerate(self.samples) if torch.equal(s["depth"], depth))
        p, q = self.poses[index]
        return p, q, torch.ones(1, device="cuda"), torch.tensor([[float(index)]], device="cuda")

    def __call__(self, depth, mask, color, shape_optimization=True):
        assert depth.dim() == 2 and mask.dtype == torch.bool and color.shape[-1] == 3
        answer = self._answer(depth)
        depth.zero_()                            # a pipeline masks its depth argument in place: the sample must survive
        return answer

    def estimate_frames(self, depth_images, masks, shape_optimization=True):
        self.frames_calls += 1
        rows = [self._answer(d) for d in depth_images]
        return tuple(torch.cat([r[j] for r in rows]) for j in range(4))

    def generate_mesh(self, latent, scale, complete_mesh=False):
        assert complete_mesh is True
        return self.ds.load_mesh(self.samples[int(latent.reshape(-1)[0].item())]["obj_path"])


@pytest.mark.parametrize("convention", ["opencv", "opengl"])
@pytest.mark.parametrize("remap", [None, ("z", "-y")], ids=["axes", "remapped"])
def test_the_annotation_itself_scores_zero(scene, convention, remap):
    from sdfest_amd.evaluation import DEFAULT_METRICS, evaluate_annotated
    extra = {} if remap is None else {"remap_x_axis": remap[0], "remap_y_axis": remap[1]}
    ds = dataset(scene, camera_convention=convention, **extra)
    result = evaluate_annotated(StandIn(ds), ds, SAMPLES, 0)
    assert sorted(result) == ["correct", "samples", "skipped", "stats"] and result["skipped"] == []
    assert [e["index"] for e in result["samples"]] == list(range(6))
    for e in result["samples"]:
        assert sorted(e["metrics"]) == sorted(DEFAULT_METRICS)
        assert e["position_error"] <= 1e-6
        assert e["rotation_error"] <= 0.05      # float32 unit quaternions through an arccos: sqrt(2 x 2^-23) rad = 0.03 deg
        assert e["metrics"]["chamfer"] <= 1e-6  # both point sets are the same samples of the same posed mesh
        assert e["correct"] == {name: 1 for name in NAMES}
    assert result["correct"] == {name: 1.0 for name in NAMES}
    assert sorted(result["stats"]) == ["all", "bottle", "mug"]
    assert sorted(result["stats"]["all"]) == sorted(list(DEFAULT_METRICS) + ["position_error", "rotation_error"])
    assert result["stats"]["mug"]["chamfer"]["mean"] <= 1e-6
    json.dumps(result)                           # what the command line writes
    # the samples were not touched by the pipeline's in-place masking
    assert all(bool(s["depth"].any()) for s in ds.samples(range(6)))


def test_a_known_offset_scores_as_computed_by_hand(scene):
    from sdfest_amd.evaluation import evaluate_annotated
    direction = np.array([2.0, -1.0, 2.0]) / 3.0
    for convention in ("opencv", "opengl"):
        ds = dataset(scene, camera_convention=convention)
        pipe = StandIn(ds, shift=0.03 * direction, turn=axis_angle([1.0, 2.0, -2.0], 7.0))
        result = evaluate_annotated(pipe, ds, SAMPLES, 0)
        for e in result["samples"]:
            assert abs(e["position_error"] - 0.03) <= 1e-6
            assert abs(e["rotation_error"] - 7.0) <= 1e-3
            assert e["correct"] == {"5deg_2cm": 0, "5deg_5cm": 0, "10deg_2cm": 0, "10deg_5cm": 1}
            assert 0.0 < e["metrics"]["chamfer"] < 0.05
        assert result["correct"] == {"5deg_2cm": 0.0, "5deg_5cm": 0.0, "10deg_2cm": 0.0, "10deg_5cm": 1.0}
        assert result["stats"]["all"]["position_error"]["mean"] == pytest.approx(0.03, abs=1e-6)
    # thresholds of the caller's own
    own = evaluate_annotated(pipe, ds, SAMPLES, 0, pose_thresholds={"loose": (8.0, 0.04), "tight": (6.0, 0.04)},
                             indices=[4, 1])
    assert [e["index"] for e in own["samples"]] == [4, 1]
    assert own["correct"] == {"loose": 1.0, "tight": 0.0}


def test_a_turn_about_a_symmetry_axis_costs_nothing(scene):
    from sdfest_amd.evaluation import evaluate_annotated
    ds = dataset(scene)
    pipe = StandIn(ds, spin=axis_angle([0.0, 1.0, 0.0], 40.0))       # about the object's own y axis
    plain = evaluate_annotated(pipe, ds, SAMPLES, 0)
    assert all(abs(e["rotation_error"] - 40.0) <= 1e-3 and e["correct"]["10deg_5cm"] == 0 for e in plain["samples"])
    result = evaluate_annotated(pipe, ds, SAMPLES, 0, symmetry_axes={"bottle": 1})
    for e in result["samples"]:
        if e["category_str"] == "bottle":
            assert e["rotation_error"] <= 0.05 and e["correct"] == {name: 1 for name in NAMES}
        else:
            assert abs(e["rotation_error"] - 40.0) <= 1e-3 and e["correct"]["10deg_5cm"] == 0
    # about another axis the turn is seen
    other = evaluate_annotated(pipe, ds, SAMPLES, 0, symmetry_axes={"bottle": 0}, indices=[3])
    assert abs(other["samples"][0]["rotation_error"] - 40.0) <= 1e-3


def test_batched_calls_and_skipped_samples_with_the_stand_in(scene):
    from sdfest_amd import NoDepthError
    from sdfest_amd.evaluation import evaluate_annotated
    ds = dataset(scene)
    pipe = StandIn(ds)
    single = evaluate_annotated(pipe, ds, SAMPLES, 0)
    assert pipe.frames_calls == 0
    batched = evaluate_annotated({"mug": pipe, "bottle": pipe}, ds, SAMPLES, 0, frames_per_call=2)
    assert pipe.frames_calls == 2                      # (0, 1) and (3, 4): runs end with the category; 2 and 5 go alone
    assert batched["samples"] == single["samples"] and batched["stats"] == single["stats"]
    only = evaluate_annotated({"bottle": pipe}, ds, SAMPLES, 0, frames_per_call=3)
    assert [e["index"] for e in only["samples"]] == [3, 4, 5] and sorted(only["stats"]) == ["all", "bottle"]
    assert [(s["index"], s["category_str"]) for s in only["skipped"]] == [(0, "mug"), (1, "mug"), (2, "mug")]
    assert all("no pipeline" in s["reason"] for s in only["skipped"])

    class NoDepth(StandIn):                            # frame 4 has no valid depth, alone or in a run
        def _answer(self, depth):
            if torch.equal(depth, self.samples[4]["depth"]):
                raise NoDepthError
            return super()._answer(depth)

    for k in (1, 3):
        result = evaluate_annotated(NoDepth(ds), ds, SAMPLES, 0, frames_per_call=k)
        assert [e["index"] for e in result["samples"]] == [0, 1, 2, 3, 5]
        assert [(s["index"], s["reason"]) for s in result["skipped"]] == [(4, "no valid depth under the mask")]


def real_pipeline(n_iter=5):
    from sdfest_amd import SDFPipeline
    from test_sdfpipeline_gpu import make_config, mug_weights, plausible_init_state
    c = redwood_scenes.CAMERA
    cfg = make_config(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], 0.005, n_iter, iso_threshold=0.0)
    return SDFPipeline(cfg, vae_state_dict=mug_weights(), init_state_dict=plausible_init_state())


def test_the_real_pipeline_entry_by_entry_and_batched(scene):
    """frames_per_call = 1 against the same steps composed by hand, bit for bit -- pose only: with shape optimisation
    d/dSDF is summed by float atomics and two runs of one call differ in the last bits.  Then frames_per_call = 3, with
    shape optimisation, through estimate_frames."""
    from sdfest_amd import evaluate_metrics, sample_points
    from sdfest_amd.evaluation import DEFAULT_METRICS, evaluate_annotated, pose_errors
    from sdfest_amd.metrics import correct_thresh
    from sdfest_amd.pointset_utils import change_orientation_camera_convention, change_position_camera_convention
    ds = dataset(scene, camera_convention="opencv")
    pipe = real_pipeline()
    result = evaluate_annotated({"mug": pipe}, ds, SAMPLES, 3, shape_optimization=False)
    assert [e["index"] for e in result["samples"]] == [0, 1, 2]
    assert [s["index"] for s in result["skipped"]] == [3, 4, 5]
    for e in result["samples"]:
        s = ds[e["index"]]
        position, orientation, scale, latent = pipe(s["depth"].clone(), s["mask"], s["color"], shape_optimization=False)
        mesh = pipe.generate_mesh(latent, scale, True)
        mesh.position, mesh.orientation = position[0], orientation[0]
        gt = ds.load_mesh(s["obj_path"])
        gt.position = change_position_camera_convention(s["position"], "opencv", "opengl")
        gt.orientation = change_orientation_camera_convention(s["quaternion"], "opencv", "opengl")
        metrics = evaluate_metrics(sample_points([gt], SAMPLES, 3)[0], sample_points([mesh], SAMPLES, 3)[0],
                                   DEFAULT_METRICS)
        assert e["metrics"] == metrics
        assert (e["position_error"], e["rotation_error"]) == pose_errors(gt.position, gt.orientation, position[0],
                                                                         orientation[0])
        assert e["correct"] == {name: correct_thresh(gt.position, position[0], gt.orientation, orientation[0],
                                                     position_threshold=m, degree_threshold=d)
                                for name, (d, m) in zip(NAMES, [(5, 0.02), (5, 0.05), (10, 0.02), (10, 0.05)])}
        assert all(np.isfinite(v) for v in metrics.values()) and e["position_error"] < 0.5

    calls = []
    frames = pipe.estimate_frames
    pipe.estimate_frames = lambda *a, **kw: (calls.append(a[0].shape[0]), frames(*a, **kw))[1]
    batched = evaluate_annotated({"mug": pipe}, ds, SAMPLES, 3, frames_per_call=3)
    assert calls == [3]
    assert [e["index"] for e in batched["samples"]] == [0, 1, 2]
    assert [(s["index"], s["category_str"]) for s in batched["skipped"]] == [(3, "bottle"), (4, "bottle"), (5, "bottle")]
    for e in batched["samples"]:
        assert all(np.isfinite(v) for v in e["metrics"].values())
        assert np.isfinite(e["position_error"]) and np.isfinite(e["rotation_error"])
    assert all(np.isfinite(v["mean"]) for v in batched["stats"]["all"].values())
