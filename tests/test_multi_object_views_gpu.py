"""GPU: SEVERAL views per object in the K-object loop (``MultiObjectRenderAndCompare(views=V)``,
``SDFPipeline.estimate_objects`` with (V,H,W) frames and (K,V,H,W) masks): K = 3 objects seen from V = 2 cameras at
160x120 -- one at the origin, one shifted and turned about 20 degrees about y -- against what a caller does today, one
multi-view call per object (``FusedRenderAndCompare`` / ``SDFPipeline.__call__`` on object k's two views)."""
import numpy as np
import pytest
import torch

import _loop_scenes as S

pytestmark = pytest.mark.gpu

T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device="cuda")
K, V, W, H, F = 3, 2, 160, 120, 150.0
ITER = 5
LRS = (1e-3, 1e-2, 1e-3, 1e-2)
NAMES = ("position", "orientation", "scale", "latent")


@pytest.fixture(scope="module")
def scene():
    """frames (V,H,W) composed per camera from renders of each object (the nearest surface wins), the instance masks
    (K,V,H,W), the cameras, and a perturbed initial estimate per object"""
    from sdfest_amd import Camera, render_depth_gpu
    dec, d = S.mug_decoder()
    cam = Camera(W, H, F, F, W / 2, H / 2, pixel_center=0.5)
    rng = np.random.default_rng(21)
    a = np.deg2rad(20.0)
    cam_pos = np.array([[0.0, 0.0, 0.0], [0.5 * np.tan(a), 0.01, -0.02]])      # the second looks back at (0, 0, -0.5)
    cam_quat = np.array([[0.0, 0.0, 0.0, 1.0], [0.0, np.sin(a / 2), 0.0, np.cos(a / 2)]])
    objs = []
    for k in range(K):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        objs.append(dict(z=d["z"][9 + k] * (0.3 + 0.1 * k), p=np.array([-0.1 + 0.1 * k, 0.02 * (k % 2) - 0.01, -0.5 - 0.02 * k]),
                         q=q, s=0.05 + 0.004 * k))
    frames, masks = [], []
    with torch.no_grad():
        for v in range(V):
            qc = cam_quat[v] * np.array([-1, -1, -1, 1.0])
            images = []
            for o in objs:
                sdf = dec.decode(T(o["z"][None]))[0, 0]
                images.append(render_depth_gpu(sdf, T(S._qrot(qc, o["p"] - cam_pos[v])), T(S._qmul(qc, o["q"])),
                                               T(1.0 / o["s"]), None, None, None, 0.005, cam))
            images = torch.stack(images)
            big = torch.where(images > 0, images, torch.full_like(images, 1e9))
            nearest, depth = big.argmin(dim=0), big.min(dim=0).values
            depth = torch.where(depth < 1e8, depth, torch.zeros_like(depth))
            frames.append(depth)
            masks.append(torch.stack([(nearest == k) & (depth > 0) for k in range(K)]))
    frames = torch.stack(frames).contiguous()                     # (V,H,W)
    masks = torch.stack(masks, dim=1).contiguous()                # (K,V,H,W)
    assert masks.sum(dim=(2, 3)).min().item() >= 200, masks.sum(dim=(2, 3))
    init = []
    for o in objs:
        q0 = o["q"] + rng.normal(0, 0.03, 4)
        init.append((o["p"] + rng.normal(0, 0.006, 3), q0 / np.linalg.norm(q0), o["s"] * 1.07, np.zeros(8)))
    p0 = T(np.stack([i[0] for i in init])); q0 = T(np.stack([i[1] for i in init]))
    s0 = T([i[2] for i in init]); z0 = T(np.stack([i[3] for i in init]))
    return dict(dec=dec, cam=cam, frames=frames, masks=masks, cam_pos=T(cam_pos), cam_quat=T(cam_quat), objs=objs,
                init=(p0, q0, s0, z0))


def config(**extra):
    return dict({"threshold": 0.005, "max_iterations": ITER, "depth_weight": 1.0, "pc_weight": 3.0}, **extra)


def object_views(scene, k):
    """object k's V images as a caller of the single loop prepares them"""
    return (scene["frames"] * scene["masks"][k]).contiguous()


@pytest.mark.parametrize("shape_opt", [False, True], ids=["pose", "shape"])
def test_rows_follow_the_single_loop_on_each_objects_views(scene, shape_opt):
    from sdfest_amd.pipeline import FusedRenderAndCompare, MultiObjectRenderAndCompare
    dec, cam = scene["dec"], scene["cam"]
    p0, q0, s0, z0 = scene["init"]
    multi = MultiObjectRenderAndCompare(dec, cam, config(), K, shape_optimization=shape_opt, graph_iterations=2, views=V)
    keep = scene["frames"].clone()
    multi.rebind(scene["frames"], scene["cam_pos"], scene["cam_quat"], masks=scene["masks"])
    assert torch.equal(scene["frames"], keep)                     # the frames are every object's: not modified
    # object-major: target[k, v] = frame v under mask (k, v)
    assert torch.equal(multi.target.view(K, V, H, W), scene["frames"][None] * scene["masks"])
    assert multi.counts.view(K, V).tolist() == scene["masks"].sum(dim=(2, 3)).tolist()
    out = [t.clone() for t in multi(p0, q0, s0, z0)]
    eager = [t.clone() for t in multi(p0, q0, s0, z0, use_graph=False)]
    torch.cuda.synchronize()
    assert multi.step.tolist() == [ITER] * K
    moved = 0.0
    for k in range(K):
        single = FusedRenderAndCompare(dec, cam, config(), object_views(scene, k), scene["cam_pos"], scene["cam_quat"],
                                       shape_optimization=shape_opt, fused_render=False)
        ref = single(p0[k:k + 1], q0[k:k + 1], s0[k:k + 1], z0[k:k + 1], use_graph=False)
        for rows in (out, eager):
            for name, a, b, lr in zip(NAMES, rows, ref, LRS):
                err = (a[k].reshape(-1) - b.reshape(-1)).abs().max().item()
                assert err <= 0.01 * lr * ITER, (k, name, err, a[k], b)
        moved = max(moved, (out[0][k] - p0[k]).abs().max().item())
        if shape_opt:
            assert out[3][k].abs().max().item() > 1e-3
        else:
            assert torch.equal(out[3][k], z0[k])
    assert moved > 1e-3
    # (K,V,H,W) images, one per object and view already: the same observation
    multi.rebind((scene["frames"][None] * scene["masks"]).contiguous(), scene["cam_pos"], scene["cam_quat"])
    again = multi(p0, q0, s0, z0)
    for a, b, lr in zip(again, out, LRS):
        assert (a - b).abs().max().item() <= 0.01 * lr * ITER


def test_views_1_is_todays_loop_bit_for_bit(scene):
    """``views=1`` launches neither volume kernel and binds (K,H,W) images as before: pose only (no float atomics),
    the rows of the constructor without the argument, bit for bit"""
    from sdfest_amd.pipeline import MultiObjectRenderAndCompare
    dec, cam = scene["dec"], scene["cam"]
    p0, q0, s0, z0 = scene["init"]
    images = (scene["frames"][0][None] * scene["masks"][:, 0]).contiguous()       # (K,H,W): the first camera
    outs = []
    for kw in ({}, {"views": 1}):
        multi = MultiObjectRenderAndCompare(dec, cam, config(), K, shape_optimization=False, **kw)
        assert multi.V == 1 and multi.sdf is multi.sdf_objects and multi.target_last is multi.target
        multi.rebind(images)
        outs.append(multi(p0, q0, s0, z0))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # ... and from the frame with 4-D masks
    multi.rebind(scene["frames"][0:1], masks=scene["masks"][:, 0:1])
    for a, b in zip(multi(p0, q0, s0, z0), outs[0]):
        assert torch.equal(a, b)


def test_limits_are_refused_at_construction(scene):
    from sdfest_amd.pipeline import MultiObjectRenderAndCompare
    dec, cam = scene["dec"], scene["cam"]
    for kw in (dict(objects=2, views=0), dict(objects=2, views=65), dict(objects=1100, views=60)):
        with pytest.raises(ValueError):
            MultiObjectRenderAndCompare(dec, cam, config(), kw["objects"], views=kw["views"])
    multi = MultiObjectRenderAndCompare(dec, cam, config(), K, views=V)
    with pytest.raises(ValueError):
        multi.rebind(scene["frames"][0:1])                        # one frame for a loop of two views
    with pytest.raises(ValueError):
        multi.rebind(scene["frames"], masks=scene["masks"][:, 0])


def test_tracking_uses_the_last_view(scene):
    from sdfest_amd.pipeline import MultiObjectRenderAndCompare
    from test_multi_object_inliers_gpu import ratio_np
    dec, cam = scene["dec"], scene["cam"]
    multi = MultiObjectRenderAndCompare(dec, cam, config(), K, shape_optimization=False, views=V, track_inliers=True)
    multi.rebind(scene["frames"], scene["cam_pos"], scene["cam_quat"], masks=scene["masks"])
    hist = []
    multi(*scene["init"], history=hist)
    torch.cuda.synchronize()
    target = multi.target.view(K, V, H, W).cpu().numpy()
    assert np.array_equal(multi.target_last.cpu().numpy(), target[:, V - 1])
    assert torch.equal(hist[-1]["depth"], multi.plan.depth.view(K, V, H, W)[:, V - 1])
    other = 0
    for i, h in enumerate(hist):
        est = h["depth"].cpu().numpy()
        want = np.array([ratio_np(target[k, V - 1], est[k]) for k in range(K)], np.float32)
        assert np.array_equal(h["inlier_ratio"].cpu().numpy().view(np.int32), want.view(np.int32)), i
        other += sum(ratio_np(target[k, 0], est[k]) != want[k] for k in range(K))
    assert other > 0                                               # (against the first view it would be another number)
    assert np.array_equal(multi.inlier_history.cpu().numpy(), np.stack([h["inlier_ratio"].cpu().numpy() for h in hist], 1))
    best = multi.best_estimates()
    assert len(best) == K and all(1 <= b[1] <= ITER for b in best)


def test_front_door_with_views(scene):
    """estimate_objects((V,H,W), (K,V,H,W), cameras) = K calls of pipeline(depth, masks[k], color, cameras)"""
    from sdfest_amd import NoDepthError, SDFPipeline
    from test_sdfpipeline_gpu import make_config, mug_weights, plausible_init_state
    frames, masks = scene["frames"], scene["masks"]
    cp, cq = scene["cam_pos"], scene["cam_quat"]
    n_iter = 4
    cfg = make_config(W, H, F, F, W / 2, H / 2, 0.005, n_iter, far_field=2.0)
    pipe = SDFPipeline(cfg, vae_state_dict=mug_weights(), init_state_dict=plausible_init_state())
    keep = frames.clone()
    out = pipe.estimate_objects(frames, masks, cp, cq)
    assert torch.equal(frames, keep)                                   # the frames are not modified
    assert [tuple(t.shape) for t in out] == [(K, 3), (K, 4), (K,), (K, 8)]
    assert pipe.best_estimates() is None                               # the default strategy keeps no bookkeeping
    color = torch.zeros((V, H, W, 3), device="cuda")
    for k in range(K):
        ref = pipe(frames.clone(), masks[k], color, camera_positions=cp, camera_orientations=cq)
        for name, a, b, lr in zip(NAMES, (out[0][k], out[1][k], out[2][k], out[3][k]), ref, LRS):
            err = (a.reshape(-1) - b.reshape(-1)).abs().max().item()
            assert err <= 0.01 * lr * n_iter, (k, name, err)
    # the next frames: nothing is built or captured again
    loop, graph = pipe._last_multi_loop, pipe._last_multi_loop.graph
    assert loop.V == V and graph is not None
    out2 = pipe.estimate_objects(frames, masks, cp, cq)
    assert pipe._last_multi_loop is loop and loop.graph is graph and len(pipe._multi_loops) == 1
    for a, b in zip(out, out2):
        assert (a - b).abs().max().item() < 1e-4
    # an (object, view) without a pixel -- in the SECOND view, which the initialisation never looks at
    empty = masks.clone(); empty[1, 1] = False
    with pytest.raises(NoDepthError):
        pipe.estimate_objects(frames, empty, cp, cq)
    # one frame and (K,H,W) masks keep working beside it, in a loop of their own
    one = pipe.estimate_objects(frames[0], masks[:, 0])
    assert [tuple(t.shape) for t in one] == [(K, 3), (K, 4), (K,), (K, 8)] and pipe._last_multi_loop.V == 1
    with pytest.raises(ValueError):
        pipe.estimate_objects(frames, masks[:, 0])

    # best_inlier_ratio: the rows stay the last iterate, the bookkeeping is there to be asked for
    tracked = SDFPipeline(dict(cfg, result_selection_strategy="best_inlier_ratio"), vae_state_dict=mug_weights(),
                          init_state_dict=plausible_init_state())
    out_t = tracked.estimate_objects(frames, masks, cp, cq)
    for a, b, lr in zip(out_t, out, LRS):
        assert (a - b).abs().max().item() <= 0.01 * lr * n_iter
    best = tracked.best_estimates()
    assert len(best) == K
    for ratio, it, params in best:
        assert 1 <= it <= n_iter and 0.0 <= ratio <= 1.0
        assert [tuple(t.shape) for t in params] == [(1, 3), (1, 4), (1,), (1, 8)]
    assert tracked._last_multi_loop.track_inliers and not loop.track_inliers

    # init_view: best has no several-view form here
    best_view = SDFPipeline(dict(cfg, init_view="best"), vae_state_dict=mug_weights(),
                            init_state_dict=plausible_init_state())
    with pytest.raises(NotImplementedError):
        best_view.estimate_objects(frames, masks, cp, cq)
