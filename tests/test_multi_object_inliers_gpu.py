"""GPU: the inlier bookkeeping of simple_setup.py:177-211 per object in the K-object loop
(``MultiObjectRenderAndCompare(track_inliers=True)``: ``sdfr_inlier_ratio_objects`` behind the tail, inside the captured
graphs) -- on the 320x240, 5-object frame of test_multi_object_gpu.py, 7 iterations.

What is compared exactly: a ratio is a quotient of two integer counts, and the count of a pixel is one IEEE float32
subtraction, division and comparison -- numpy on the very images the loop rendered gives the same bits."""
import numpy as np
import pytest
import torch

from test_multi_object_gpu import T, frame  # noqa: F401  (the module-scoped scene, built once for this file)

pytestmark = pytest.mark.gpu

ITER = 7
THR = np.float32(0.03)      # the default relative_inlier_threshold, as the kernel receives it
LRS = (1e-3, 1e-2, 1e-3, 1e-2)


def ratio_np(din, est):
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(din - est) / din
        return np.float32(np.count_nonzero(rel < THR)) / np.float32(np.count_nonzero(din))


def first_strict_maximum(ratios):
    """(ratio, 1-based iteration) as :203-210 pick it: the first counts, then strictly greater only"""
    best = None
    for i, r in enumerate(ratios):
        if best is None or r > best[0]:
            best = (r, i + 1)
    return best


def same(a, b):
    """bit for bit, NaN included"""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("shape_opt", [False, True], ids=["pose", "shape"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_bookkeeping_per_object(frame, shape_opt, use_graph):
    from sdfest_amd.pipeline import FusedRenderAndCompare, MultiObjectRenderAndCompare, preprocess_depth
    dec, cam, depth, masks, init, _ = frame
    K = masks.shape[0]
    cfg = {"threshold": 0.005, "max_iterations": ITER, "depth_weight": 1.0, "pc_weight": 3.0}
    frames = depth[None].expand(K, -1, -1).contiguous()
    preprocess_depth(frames, masks, 2.0)
    p0 = T(np.stack([i[0] for i in init])); q0 = T(np.stack([i[1] for i in init]))
    s0 = T([i[2] for i in init]); z0 = T(np.stack([i[3] for i in init]))

    multi = MultiObjectRenderAndCompare(dec, cam, cfg, K, shape_optimization=shape_opt, graph_iterations=3,
                                        track_inliers=True)
    assert multi.track_inliers and multi.inlier_history.shape == (K, ITER)
    multi.rebind(frames)
    hist = []
    out = [t.clone() for t in multi(p0, q0, s0, z0, use_graph=use_graph, history=hist)]
    torch.cuda.synchronize()
    assert len(hist) == ITER and multi.step.tolist() == [ITER] * K

    # off: nothing is launched, nothing is kept -- and the estimate does not depend on the bookkeeping
    plain = MultiObjectRenderAndCompare(dec, cam, cfg, K, shape_optimization=shape_opt, graph_iterations=3)
    assert not plain.track_inliers and plain.best_estimates() is None
    plain.rebind(frames)
    hist_plain = []
    out_plain = plain(p0, q0, s0, z0, use_graph=use_graph, history=hist_plain)
    assert "inlier_ratio" not in hist_plain[0] and "depth" not in hist_plain[0]
    assert not plain.inlier_history.any() and not plain.best_state.any()
    for a, b, lr in zip(out, out_plain, LRS):
        assert (a - b).abs().max().item() <= 0.01 * lr * ITER
        if not shape_opt:      # pose only: no float atomics anywhere
            assert torch.equal(a, b)

    # every recorded ratio is the ratio of the images the iteration rendered
    target = frames.cpu().numpy()
    ratios = np.zeros((ITER, K), np.float32)
    for i, h in enumerate(hist):
        est = h["depth"].cpu().numpy()
        assert est.shape == target.shape and h["inlier_ratio"].shape == (K,)
        for k in range(K):
            ratios[i, k] = ratio_np(target[k], est[k])
        assert np.array_equal(h["inlier_ratio"].cpu().numpy().view(np.int32), ratios[i].view(np.int32)), i
    assert np.array_equal(multi.inlier_history.cpu().numpy().view(np.int32), ratios.T.view(np.int32))
    assert np.isfinite(ratios).all() and ratios.max() <= 1.0 and len(np.unique(ratios)) > K      # (a scene where it moves)

    best = multi.best_estimates()
    assert len(best) == K
    for k in range(K):
        r, it = first_strict_maximum(ratios[:, k])
        assert best[k][0] == float(r) and best[k][1] == it, (k, best[k][:2], r, it)
        row = hist[it - 1]["params"][k]
        got = best[k][2]
        assert [tuple(t.shape) for t in got] == [(1, 3), (1, 4), (1,), (1, 8)]
        assert same(torch.cat([t.reshape(-1) for t in got]), row), k
    state = multi.best_state.clone()
    history = multi.inlier_history.clone()
    best_params = multi.best_params.clone()

    if not shape_opt:
        # the single-object loop with its own bookkeeping (sdfr_inlier_ratio), in the K-object loop's two-launch form
        for k in range(K):
            single = FusedRenderAndCompare(dec, cam, cfg, frames[k:k + 1].contiguous(), shape_optimization=False,
                                           fused_render=False, track_inliers=True)
            single(p0[k:k + 1], q0[k:k + 1], s0[k:k + 1], z0[k:k + 1], use_graph=False)
            assert torch.equal(single.inlier_history, history[k]), k
            assert torch.equal(single.best_state, state[k]), k
            assert torch.equal(single.best_params, best_params[k]), k

    # Pose only, every run is the same bits.  With shape optimisation the d/dSDF volumes are summed with float atomics
    # and two runs differ within the project's yardstick, 1 % of an Adam step per iteration: a pixel changes sides only
    # if its relative error lies within ~1e-5 of the threshold, so far fewer than one pixel in a hundred may
    def same_bookkeeping(h, s, perm=None):
        h0, s0_ = (history, state) if perm is None else (history[perm], state[perm])
        if not shape_opt:
            return same(h, h0) and same(s, s0_)
        return (h - h0).abs().max().item() <= 0.01 and (s[:, 0] - s0_[:, 0]).abs().max().item() <= 0.01

    # a second run resets the bookkeeping and replays what the first captured (whole graphs of 3 iterations, then 1)
    graph = multi.graph
    out2 = multi(p0, q0, s0, z0, use_graph=use_graph)
    torch.cuda.synchronize()
    assert multi.graph is graph and (graph is not None) == use_graph
    assert same_bookkeeping(multi.inlier_history, multi.best_state)
    for a, b, lr in zip(out2, out, LRS):
        assert (a - b).abs().max().item() <= 0.01 * lr * ITER

    # the next frame, the objects in another order: the rows permute
    perm = torch.tensor([2, 0, 4, 1, 3], device="cuda")
    multi.rebind(frames[perm].contiguous())
    multi(p0[perm], q0[perm], s0[perm], z0[perm], use_graph=use_graph)
    torch.cuda.synchronize()
    assert multi.graph is graph
    assert same_bookkeeping(multi.inlier_history, multi.best_state, perm)
    if not shape_opt:
        assert same(multi.best_params, best_params[perm])


def test_default_follows_the_result_selection_strategy(frame):
    from sdfest_amd.pipeline import MultiObjectRenderAndCompare
    dec, cam = frame[0], frame[1]
    cfg = {"threshold": 0.005, "max_iterations": 2, "depth_weight": 1.0, "pc_weight": 3.0}
    assert not MultiObjectRenderAndCompare(dec, cam, cfg, 2).track_inliers
    on = MultiObjectRenderAndCompare(dec, cam, dict(cfg, result_selection_strategy="best_inlier_ratio"), 2)
    assert on.track_inliers and on.best_estimates() == [None, None]
    assert not MultiObjectRenderAndCompare(dec, cam, dict(cfg, result_selection_strategy="best_inlier_ratio"), 2,
                                           track_inliers=False).track_inliers
    with pytest.raises(ValueError):
        MultiObjectRenderAndCompare(dec, cam, dict(cfg, result_selection_strategy="median"), 2)
