"""GPU: ``step_log: true`` at the front door -- the trajectory of a call, the reference's log pickle and animation
folder -- on the mug configuration with the fixed-init stand-in of tests/test_sdfpipeline_gpu.py (G7 run C's two
160x120 views), 3 iterations."""
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from test_sdfpipeline_gpu import T, make_config, mug_weights

pytestmark = pytest.mark.gpu

N_ITER = 3


@pytest.fixture(scope="module")
def g7():
    d = np.load(os.path.join(GOLDEN, "loop_g7.npz"))
    return {k: d[k] for k in d.files}


def build(g7, n_iter=N_ITER, deterministic=False, **extra):
    """deterministic: the loop's d/dSDF as integer sums (``SDF_GRAD_DETERMINISTIC | BWD_SMALL_TILES``), which the
    config cannot ask for: ``sdf_grad_mode`` is a plain attribute the pipeline reads when it builds its loop"""
    from sdfest_amd import SDFPipeline
    from sdfest_amd.differentiable_renderer import BWD_SMALL_TILES, SDF_GRAD_DETERMINISTIC
    W, H = int(g7["c_W"]), int(g7["c_H"])
    assert (W, H) == (160, 120) and g7["c_depth_images"].shape[0] == 2
    cfg = make_config(W, H, float(g7["c_fx"]), float(g7["c_fy"]), float(g7["c_cx"]), float(g7["c_cy"]), float(g7["thr"]),
                      n_iter, far_field=50.0, **extra)
    init = g7["c_init"]
    fixed_init = lambda *a: (T(init[None, 8:]), T(init[None, 0:3]), T(init[7:8]), T(init[None, 3:7]))
    pipe = SDFPipeline(cfg, vae_state_dict=mug_weights(), init_network=fixed_init)
    if deterministic:
        pipe.sdf_grad_mode = SDF_GRAD_DETERMINISTIC | BWD_SMALL_TILES
    return pipe


def observation(g7):
    depth = T(g7["c_depth_images"])
    masks = torch.ones_like(depth, dtype=torch.bool)
    masks[:, :5] = False                                   # (something for the preprocessing to remove)
    color = torch.zeros(depth.shape + (3,), device="cuda")
    color[..., 1] = 0.5
    cams = dict(camera_positions=T(g7["c_cam_pos"]), camera_orientations=T(g7["c_cam_quat"]))
    return depth, masks, color, cams


@pytest.fixture(scope="module")
def run(g7, tmp_path_factory):
    """calls without the key and with it (a log and an animation), pose-only and with shape optimisation: shared,
    unchanged, by the tests below"""
    folder = tmp_path_factory.mktemp("step_log")
    depth, masks, color, cams = observation(g7)
    plain_pipe = build(g7)
    plain = plain_pipe(depth.clone(), masks, color, **cams)
    plain_pose = plain_pipe(depth.clone(), masks, color, shape_optimization=False, **cams)
    plain_again = build(g7)(depth.clone(), masks, color, **cams)
    pipe = build(g7, step_log=True)
    log_path, animation_path = str(folder / "log.pkl"), str(folder / "animation")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        logged_pose = pipe(depth.clone(), masks, color, shape_optimization=False, log_path=str(folder / "pose.pkl"),
                           **cams)
        pose_rows = pipe.last_trajectory()
        logged = pipe(depth.clone(), masks, color, log_path=log_path, animation_path=animation_path, **cams)
    torch.cuda.synchronize()
    assert not [x for x in w if "ignored" in str(x.message)]
    return dict(plain=plain, plain_again=plain_again, logged=logged, plain_pose=plain_pose, logged_pose=logged_pose, pose_rows=pose_rows,
                pipe=pipe, log_path=log_path, animation_path=animation_path)


def flat(estimate):
    return torch.cat([t.reshape(-1) for t in estimate])


def test_estimate_is_bitwise_the_one_without_the_key(run):
    """Pose-only, every launch of the loop sums in a fixed order: the 4-tuple with ``step_log`` is bitwise the one
    without."""
    for a, b in zip(run["plain_pose"], run["logged_pose"]):
        assert a.shape == b.shape and torch.equal(a, b)
    for rows, out in zip(run["pose_rows"], run["logged_pose"]):
        assert torch.equal(rows[-1].reshape(-1), out.reshape(-1))
    assert torch.equal(run["pose_rows"][3][0], run["pose_rows"][3][-1])          # pose-only: the latent stays


@pytest.mark.parametrize("n_iter", [N_ITER, 7])
@pytest.mark.parametrize("shape_optimization", [True, False])
def test_recording_changes_no_bit_of_a_reproducible_run(g7, n_iter, shape_optimization):
    """With shape optimisation the comparison needs a loop whose own bits repeat: d/dSDF summed as integers.  Then the
    4-tuple with ``step_log`` is bitwise the one without, also over 7 iterations, where the plain call replays the
    graph of ``graph_iterations`` = 5 iterations and two single ones while a history makes every iteration a single
    replay (``_graphs.run``) -- the one difference recording makes to what is launched.  Pose-only at 7 iterations the
    default loop is compared the same way."""
    depth, masks, color, cams = observation(g7)
    det = shape_optimization
    plain_pipe, pipe = build(g7, n_iter, det), build(g7, n_iter, det, step_log=True)
    kw = dict(shape_optimization=shape_optimization, **cams)
    plain = plain_pipe(depth.clone(), masks, color, **kw)
    logged = pipe(depth.clone(), masks, color, **kw)
    again = plain_pipe(depth.clone(), masks, color, **kw)
    loop = plain_pipe._last_loop
    assert loop.det == det and loop.graph is not None and pipe._last_loop.graph is not None
    assert (loop.graph_many is not None) and loop.graph_iterations == 5        # 7 iterations: 5 + 1 + 1 without a history
    assert torch.equal(flat(plain), flat(again))                               # the run repeats its own bits
    assert torch.equal(flat(plain), flat(logged))
    rows = pipe.last_trajectory()
    assert rows[0].shape[0] == n_iter + 1 and torch.equal(flat([r[-1] for r in rows]), flat(logged))
    assert torch.equal(rows[3][0], rows[3][-1]) != shape_optimization          # the latent moves iff it is optimised


def test_default_shape_optimised_run_within_its_own_scatter(run):
    """The default loop adds d/dSDF with float atomics, so two identical calls WITHOUT the key differ in the last bits
    and no recorded run can be bitwise a plain one.  The bound, 1e-6 on every component, from the arithmetic: the order
    of a float sum of n terms moves it by about sqrt(n) 2^-24 of its size -- 1e-6 ... 1e-5 for the up to 4096
    contributions of a voxel --, an Adam step is lr m / (sqrt(v) + eps) <= lr = 1e-2 and moves by at most that
    relative amount of lr when its gradients do, and there are 3 steps: 3 x 1e-2 x 1e-5 = 3e-7.  Two plain calls scatter
    as much as a plain and a recorded one do (measured on an MI355X: 1.3e-8 between two plain calls, 2.2e-8 between a
    plain and a recorded one; both are printed), and both are held to the bound."""
    scatter = (flat(run["plain"]) - flat(run["plain_again"])).abs().max().item()
    recorded = (flat(run["plain"]) - flat(run["logged"])).abs().max().item()
    print(f"3 iterations, shape optimisation: two plain calls differ by {scatter:.3e}, plain and recorded by {recorded:.3e}")
    assert scatter <= 1e-6
    assert recorded <= 1e-6


def test_last_trajectory(run, g7):
    pos, quat, scale, latent = run["pipe"].last_trajectory()
    assert (tuple(pos.shape), tuple(quat.shape), tuple(scale.shape), tuple(latent.shape)) == (
        (N_ITER + 1, 3), (N_ITER + 1, 4), (N_ITER + 1,), (N_ITER + 1, 8))
    for rows, out in zip((pos, quat, scale, latent), run["logged"]):
        assert torch.equal(rows[-1].reshape(-1), out.reshape(-1))
    init = T(g7["c_init"])
    assert torch.equal(torch.cat([pos[0], quat[0], scale[0:1], latent[0]]), init)
    assert not torch.equal(pos[1], pos[0]) and not torch.equal(latent[2], latent[1])     # the loop moved


def test_log_pickle_is_the_references(run, g7):
    with open(run["log_path"], "rb") as f:
        data = pickle.load(f)
    assert sorted(data) == ["config", "log"] and data["config"]["step_log"] is True
    log = data["log"]
    assert len(log) == 2 + N_ITER
    assert sorted(log[0]) == ["camera_orientations", "camera_positions", "color_images", "depth_images", "masks",
                              "timestamp"]
    assert tuple(log[0]["depth_images"].shape) == (2, 120, 160) and tuple(log[0]["masks"].shape) == (2, 120, 160)
    assert not log[0]["depth_images"][:, :5].any()                       # as preprocessed
    state_keys = ["latent_shape", "orientation", "position", "scale_inv", "timestamp"]
    assert sorted(log[1]) == sorted(state_keys + ["camera_orientations", "camera_positions"])
    pos, quat, scale, latent = (t.cpu() for t in run["pipe"].last_trajectory())
    for t, entry in enumerate(log[1:]):
        if t:
            assert sorted(entry) == state_keys
        assert (tuple(entry["position"].shape), tuple(entry["orientation"].shape), tuple(entry["scale_inv"].shape),
                tuple(entry["latent_shape"].shape)) == ((1, 3), (1, 4), (1,), (1, 8))
        assert torch.equal(entry["position"][0], pos[t]) and torch.equal(entry["orientation"][0], quat[t])
        assert torch.equal(entry["latent_shape"][0], latent[t]) and torch.equal(entry["scale_inv"], 1 / scale[t:t + 1])
    for entry in log:
        for v in entry.values():
            assert not isinstance(v, torch.Tensor) or v.device.type == "cpu"
    stamps = [e["timestamp"] for e in log]
    assert all(isinstance(s, float) and s >= 0 for s in stamps)
    assert all(b >= a for a, b in zip(stamps, stamps[1:])) and stamps[-1] > stamps[1]


def test_animation_folder(run):
    from PIL import Image
    from sdfest_amd import render_depth_batch, shade_frames
    from sdfest_amd.pipeline import quaternion_apply, quaternion_invert, quaternion_multiply
    root = run["animation_path"]
    expect = sorted(["depth", "depth_error", "sdf", "color_input.png", "depth_input.png", "mask.png",
                     "preprocessed_depth_input.png", "depth.gif", "depth_error.gif", "sdf.gif"])
    assert sorted(os.listdir(root)) == expect
    for name in ("depth", "depth_error", "sdf"):
        assert sorted(os.listdir(os.path.join(root, name))) == [f"{i:06}.png" for i in range(1, N_ITER + 1)]
        for i in range(1, N_ITER + 1):
            img = Image.open(os.path.join(root, name, f"{i:06}.png"))
            assert img.size == (160, 120) and img.mode == "RGB"
        gif = Image.open(os.path.join(root, f"{name}.gif"))
        assert gif.size == (160, 120) and 1 <= gif.n_frames <= N_ITER      # (PIL merges frames that quantise alike)
    for name in ("color_input.png", "depth_input.png", "mask.png", "preprocessed_depth_input.png"):
        assert Image.open(os.path.join(root, name)).size == (160, 120)
    # depth/000002.png is exactly what shade_frames gives for state 2
    pipe = run["pipe"]
    pos, quat, scale, latent = (t[2:3] for t in pipe.last_trajectory())
    r = pipe._trajectory
    q_w2c = quaternion_invert(r.cam_quat[0])
    sdf = pipe.vae.decode(latent)[0, 0]
    depth = render_depth_batch(sdf, quaternion_apply(q_w2c, pos - r.cam_pos[0]).contiguous(),
                               quaternion_multiply(q_w2c[None], quat).contiguous(), (1 / scale).contiguous(),
                               pipe.config["threshold"], pipe.cam)
    frame = shade_frames(depth, None, None, None, None, pipe.cam, target=r.target[0:1], outputs=("depth",))["depth"][0]
    assert (depth != 0).sum() > 100
    decoded = np.asarray(Image.open(os.path.join(root, "depth", "000002.png")))
    assert np.array_equal(decoded, frame.cpu().numpy())


def test_trajectory_frames_equal_single_state_calls(run):
    from sdfest_amd import render_depth_batch, shade_frames, trajectory_frames
    from sdfest_amd.pipeline import quaternion_apply, quaternion_invert, quaternion_multiply
    from sdfest_amd.visualization import canonical_view
    pipe = run["pipe"]
    r = pipe._trajectory
    states = pipe.last_trajectory()
    for view in (0, 1):
        frames = trajectory_frames(pipe, states, r.target, r.cam_pos, r.cam_quat, view=view)
        assert sorted(frames) == ["depth", "depth_error", "sdf"]
        again = pipe.render_trajectory(view=view)
        q_w2c = quaternion_invert(r.cam_quat[view])
        for t in range(N_ITER + 1):
            pos, quat, scale, latent = (s[t:t + 1] for s in states)
            sdf = pipe.vae.decode(latent)[0, 0]
            args = (quaternion_apply(q_w2c, pos - r.cam_pos[view]).contiguous(),
                    quaternion_multiply(q_w2c[None], quat).contiguous(), (1 / scale).contiguous())
            depth = render_depth_batch(sdf, *args, pipe.config["threshold"], pipe.cam)
            seen = shade_frames(depth, None, None, None, None, pipe.cam, target=r.target[view:view + 1],
                                outputs=("depth", "depth_error"))
            can = canonical_view(pipe.cam, 1, depth.device)
            c_depth = render_depth_batch(sdf, *can, pipe.config["threshold"], pipe.cam)
            shape = shade_frames(c_depth, sdf, *can, pipe.cam, outputs=("shaded",))["shaded"]
            assert (c_depth != 0).sum() > 200 and (depth != 0).sum() > 100       # the object is in both pictures
            assert torch.equal(frames["depth"][t], seen["depth"][0]), (view, t)
            assert torch.equal(frames["depth_error"][t], seen["depth_error"][0]), (view, t)
            assert torch.equal(frames["sdf"][t], shape[0]), (view, t)
        for name in frames:
            assert frames[name].shape == (N_ITER + 1, 120, 160, 3) and frames[name].dtype == torch.uint8
            assert torch.equal(frames[name], again[name])
    # a history (the loop's list of per-iteration dicts) is taken as its stacked tensors are
    from_history = trajectory_frames(pipe, list(r.history), r.target, r.cam_pos, r.cam_quat, view=1)
    assert torch.equal(from_history["sdf"], frames["sdf"][1:])


def test_trajectory_render_is_the_loops_own_render(run):
    """Independent of this file's own camera arithmetic: the loop's last render -- ``plan.depth``, the estimate BEFORE
    the last step as the loop itself posed it in each of its views (``sdfr_pose_to_views``) -- against
    ``trajectory_depth`` of row N_ITER - 1.  Both are float32 renders of the same grid; the poses come from two
    implementations of the same three expressions, so they agree to a few ulp and the depths to ~1e-6: at most 1 % of
    the hit pixels may fall on the other side of their hit test, the median difference is at most 1e-5.  And the
    estimate lies on the observation it was fitted to."""
    from sdfest_amd import trajectory_frames
    from sdfest_amd.visualization import trajectory_depth
    pipe = run["pipe"]
    r, loop = pipe._trajectory, pipe._last_loop
    states = pipe.last_trajectory()
    for view in (0, 1):
        _, depth = trajectory_depth(pipe, states, r.cam_pos, r.cam_quat, view=view)
        own, mine = loop.plan.depth[view], depth[N_ITER - 1]
        hit_own, hit_mine = own != 0, mine != 0
        both = hit_own & hit_mine
        assert both.sum().item() > 100
        mismatch = (hit_own ^ hit_mine).sum().item() / hit_own.sum().item()
        median = (own - mine).abs()[both].median().item()
        observed = r.target[view] != 0
        iou = (hit_mine & observed).sum().item() / (hit_mine | observed).sum().item()
        print(f"view {view}: hit pixels {int(hit_own.sum())}, on the other side {100 * mismatch:.2f} %, median depth "
              f"difference {median:.2e}, IoU with the observation {iou:.2f}")
        assert mismatch <= 0.01 and median <= 1e-5
        assert iou > 0.3
        # ... and the frames are pictures of that depth: background exactly where it has none
        frame = trajectory_frames(pipe, states, r.target, r.cam_pos, r.cam_quat, view=view)["depth"][N_ITER - 1]
        assert torch.equal((frame != 255).any(-1), hit_mine)


def test_forms_without_a_single_trajectory_are_refused(g7, tmp_path):
    depth, masks, color, cams = observation(g7)
    pipe = build(g7, step_log=True, orientation_hypotheses=2)
    with pytest.raises(NotImplementedError, match="orientation_hypotheses"):
        pipe(depth.clone(), masks, color, log_path=str(tmp_path / "log.pkl"), **cams)
    pipe = build(g7, step_log=True)
    with pytest.raises(NotImplementedError, match="estimate_objects"):
        pipe.estimate_objects(depth[0].clone(), masks[:1], animation_path=str(tmp_path / "animation"))
    with pytest.raises(NotImplementedError, match="estimate_frames"):
        pipe.estimate_frames(depth.clone(), masks, log_path=str(tmp_path / "log.pkl"))
    assert not os.listdir(tmp_path)
    with pytest.raises(RuntimeError, match="step_log"):
        build(g7).last_trajectory()
    # a call that records nothing leaves no earlier call's trajectory behind
    pipe(depth.clone(), masks, color, shape_optimization=False, **cams)
    assert pipe.last_trajectory()[0].shape == (N_ITER + 1, 3)
    pipe.config["orientation_hypotheses"] = 2
    with pytest.raises(NotImplementedError):
        pipe(depth.clone(), masks, color, log_path=str(tmp_path / "log.pkl"), **cams)
    with pytest.raises(RuntimeError, match="no trajectory"):
        pipe.last_trajectory()
    with pytest.raises(RuntimeError, match="no trajectory"):
        pipe.render_trajectory()
