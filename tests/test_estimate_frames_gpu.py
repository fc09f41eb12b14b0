"""GPU: ``SDFPipeline.estimate_frames`` -- K DIFFERENT frames with one object each, refined side by side as the K rows
of ``estimate_objects``' loop.  The scene recipe of tests/test_multi_object_views_gpu.py with one camera: K = 3 mugs
at 160x120, 5 iterations; the composed frame with its K instance masks, and K frames that show one object each."""
import numpy as np
import pytest
import torch

import _loop_scenes as S

pytestmark = pytest.mark.gpu

T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device="cuda")
K, W, H, F = 3, 160, 120, 150.0
ITER = 5
LRS = (1e-3, 1e-2, 1e-3, 1e-2)
NAMES = ("position", "orientation", "scale", "latent")


@pytest.fixture(scope="module")
def scene():
    """images (K,H,W): object k alone in front of the camera at the origin; frame (H,W): all of them, the nearest
    surface wins, with the instance masks (K,H,W)"""
    from sdfest_amd import Camera, render_depth_gpu
    dec, d = S.mug_decoder()
    cam = Camera(W, H, F, F, W / 2, H / 2, pixel_center=0.5)
    rng = np.random.default_rng(21)
    images = []
    with torch.no_grad():
        for k in range(K):
            q = rng.normal(size=4); q /= np.linalg.norm(q)
            z = d["z"][9 + k] * (0.3 + 0.1 * k)
            p = np.array([-0.1 + 0.1 * k, 0.02 * (k % 2) - 0.01, -0.5 - 0.02 * k])
            sdf = dec.decode(T(z[None]))[0, 0]
            images.append(render_depth_gpu(sdf, T(p), T(q), T(1.0 / (0.05 + 0.004 * k)), None, None, None, 0.005, cam))
    images = torch.stack(images).contiguous()
    big = torch.where(images > 0, images, torch.full_like(images, 1e9))
    nearest, depth = big.argmin(dim=0), big.min(dim=0).values
    frame = torch.where(depth < 1e8, depth, torch.zeros_like(depth)).contiguous()
    masks = torch.stack([(nearest == k) & (frame > 0) for k in range(K)]).contiguous()
    assert masks.sum(dim=(1, 2)).min().item() >= 200 and (images > 0).sum(dim=(1, 2)).min().item() >= 200
    return dict(images=images, frame=frame, masks=masks)


def pipeline(**extra):
    from sdfest_amd import SDFPipeline
    from test_sdfpipeline_gpu import make_config, mug_weights, plausible_init_state
    cfg = make_config(W, H, F, F, W / 2, H / 2, 0.005, ITER, **dict({"far_field": 2.0}, **extra))
    return SDFPipeline(cfg, vae_state_dict=mug_weights(), init_state_dict=plausible_init_state())


@pytest.mark.parametrize("shape_opt", [False, True], ids=["pose", "shape"])
def test_copies_of_one_frame_are_estimate_objects_bit_for_bit(scene, shape_opt):
    """pose only: the same bits (the loop, its initialisation and its images are the same).  With shape optimisation
    d/dSDF is summed by float atomics, so two runs of ONE call already differ in the last bits: those rows are held to
    the bound the project holds rows to, 1 % of an Adam step per iteration."""
    pipe = pipeline()
    frame, masks = scene["frame"], scene["masks"]
    keep = frame.clone()
    ref = [t.clone() for t in pipe.estimate_objects(frame, masks, shape_optimization=shape_opt)]
    assert torch.equal(frame, keep)
    loop = pipe._last_multi_loop
    copies = frame[None].repeat(K, 1, 1).contiguous()
    out = pipe.estimate_frames(copies, masks, shape_optimization=shape_opt)
    torch.cuda.synchronize()
    assert pipe._last_multi_loop is loop and len(pipe._multi_loops) == 1      # the same cached loop serves both calls
    assert [tuple(t.shape) for t in out] == [(K, 3), (K, 4), (K,), (K, 8)]
    for name, a, b, lr in zip(NAMES, out, ref, LRS):
        if shape_opt:
            assert (a - b).abs().max().item() <= 0.01 * lr * ITER, name
        else:
            assert torch.equal(a, b), name
    assert (out[0] - out[0][0]).abs().max().item() > 1e-2                      # three different objects
    # depth is masked (and far-field clipped) in place, as in __call__
    assert torch.equal(copies, frame[None] * masks)
    assert pipe.best_estimates() is None                                       # the default strategy keeps no bookkeeping


def test_different_frames_follow_estimate_objects_row_by_row(scene):
    pipe = pipeline()
    images = scene["images"]
    masks = images > 0
    out = [t.clone() for t in pipe.estimate_frames(images.clone(), masks)]
    for k in range(K):
        ref = pipe.estimate_objects(images[k], masks[k][None])
        for name, a, b, lr in zip(NAMES, out, ref, LRS):
            err = (a[k].reshape(-1) - b.reshape(-1)).abs().max().item()
            print(f"row {k} {name}: {err / (lr * ITER):.2e} of lr x iterations")
            assert err <= 0.01 * lr * ITER, (k, name, err)
    # the rows moved, and not together
    assert (out[0][0] - out[0][2]).abs().max().item() > 1e-2
    # masks that cut into the frames: the masked images are what the loop sees
    half = masks.clone()
    half[:, :, : W // 2 - 20] = False
    depth = images.clone()
    pipe.estimate_frames(depth, half)
    assert torch.equal(depth, images * half)
    assert torch.equal(pipe._last_multi_loop.target, depth)
    # a far field clips in place too
    near = pipeline(far_field=0.53)
    depth = images.clone()
    near.estimate_frames(depth, masks)
    assert torch.equal(depth, torch.where(images > 0.53, torch.zeros_like(images), images))
    assert (depth != images).any() and (depth > 0).flatten(1).any(1).all()


def test_best_estimates_errors_and_empty_masks(scene):
    from sdfest_amd import NoDepthError
    images = scene["images"]
    masks = images > 0
    tracked = pipeline(result_selection_strategy="best_inlier_ratio")
    out = tracked.estimate_frames(images.clone(), masks)
    best = tracked.best_estimates()
    assert len(best) == K
    for ratio, it, params in best:
        assert 1 <= it <= ITER and 0.0 <= ratio <= 1.0
        assert [tuple(t.shape) for t in params] == [(1, 3), (1, 4), (1,), (1, 8)]
    assert [tuple(t.shape) for t in out] == [(K, 3), (K, 4), (K,), (K, 8)]
    # one frame is a batch of one
    one = tracked.estimate_frames(images[1:2].clone(), masks[1:2])
    assert [tuple(t.shape) for t in one] == [(1, 3), (1, 4), (1,), (1, 8)] and len(tracked.best_estimates()) == 1
    for depth, m in ((images[0], masks[0]), (images.clone(), masks[:2]), (images.clone(), masks[:, :-1]),
                     (images[:, :-8].clone(), masks[:, :-8]), (images[None].clone(), masks[None])):
        with pytest.raises(ValueError):
            tracked.estimate_frames(depth, m)
    empty = masks.clone()
    empty[1] = False
    with pytest.raises(NoDepthError):
        tracked.estimate_frames(images.clone(), empty)
    # ... and the pipeline goes on with the next frames
    again = tracked.estimate_frames(images.clone(), masks)
    for a, b, lr in zip(again, out, LRS):
        assert (a - b).abs().max().item() <= 0.01 * lr * ITER
