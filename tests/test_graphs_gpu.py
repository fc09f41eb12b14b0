"""GPU: the one capture path of the loops (``_graphs.capture``) on a toy body, its failure path -- an ordinary host
exception under capture -- and the same failure inside a real loop, which must leave the loop as it was."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN

pytestmark = pytest.mark.gpu


def _x():
    return torch.arange(16, dtype=torch.float32, device="cuda")


def test_capture_restores_the_state_and_replays():
    from sdfest_amd._graphs import capture
    x, x0 = _x(), _x()
    dev = x.device

    def body():
        x.add_(1)

    def three():
        for _ in range(3):
            body()

    one, many = capture(dev, (body, three), body, state=(x,))
    torch.cuda.synchronize()
    assert torch.equal(x, x0)               # the warm-up ran, neither it nor the captures left a trace
    one.replay()
    assert torch.equal(x, x0 + 1)
    one.replay()
    assert torch.equal(x, x0 + 2)
    many.replay()
    assert torch.equal(x, x0 + 5)


def test_a_failed_capture_hands_out_nothing_and_the_next_one_works():
    from sdfest_amd._graphs import capture
    x, x0 = _x(), _x()
    dev = x.device
    calls = []

    def failing():
        x.add_(1)
        calls.append(1)
        if len(calls) == 2:                 # the warm-up passes; the first capture does not
            raise RuntimeError("host error under capture")

    graphs = None
    with pytest.raises(RuntimeError, match="host error under capture"):
        graphs = capture(dev, (failing, failing), failing, state=(x,))
    torch.cuda.synchronize()
    assert graphs is None and len(calls) == 2      # (the second sequence was never tried)
    assert torch.equal(x, x0)
    assert not torch.cuda.is_current_stream_capturing()

    def body():
        x.add_(1)

    one, = capture(dev, (body,), body, state=(x,))
    assert torch.equal(x, x0)
    one.replay()
    assert torch.equal(x, x0 + 1)


def test_a_loop_whose_capture_failed_captures_afresh():
    """``FusedRenderAndCompare`` with ``iteration`` raising once under capture: no graph is kept (``loop.graph`` used to
    stay set, and the next call replayed the unfinished graph), the next call captures and gives a fresh object's
    result bit for bit (pose only: no float atomics on the way)"""
    import _loop_scenes as S
    from sdfest_amd import Camera
    from sdfest_amd.pipeline import FusedRenderAndCompare
    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device="cuda")
    dec, _ = S.mug_decoder()
    g7 = np.load(os.path.join(GOLDEN, "loop_g7.npz"))      # run C: 2 views, 160x120 (test_rebind_gpu.py)
    cam = Camera(int(g7["c_W"]), int(g7["c_H"]), float(g7["c_fx"]), float(g7["c_fy"]), float(g7["c_cx"]),
                 float(g7["c_cy"]), pixel_center=0.5)
    init = g7["c_init"]
    init = (T(init[None, 0:3]), T(init[None, 3:7]), T(init[7:8]), T(init[None, 8:]))
    cfg = {"threshold": float(g7["thr"]), "max_iterations": 7, "depth_weight": 1.0, "pc_weight": 3.0,
           "result_selection_strategy": "best_inlier_ratio"}

    def fresh():
        return FusedRenderAndCompare(dec, cam, cfg, T(g7["c_depth_images"]), T(g7["c_cam_pos"]), T(g7["c_cam_quat"]),
                                     graph_iterations=3, shape_optimization=False)

    def result(loop):
        out = loop(*init)
        torch.cuda.synchronize()
        return [t.clone() for t in out] + [loop.inlier_history.clone(), loop.best_state.clone(), loop.best_params.clone()]

    ref = result(fresh())
    loop = fresh()
    iteration, calls = loop.iteration, []

    def failing_once():
        calls.append(1)
        iteration()
        if len(calls) == 2:                 # 1: the warm-up, 2: the capture of the one-iteration graph
            raise RuntimeError("host error under capture")

    loop.iteration = failing_once
    with pytest.raises(RuntimeError, match="host error under capture"):
        loop(*init)
    assert len(calls) == 2
    assert loop.graph is None and loop.graph_many is None and len(loop._graphs) == 0
    got = result(loop)
    assert loop.graph is not None and loop.graph_many is not None and len(loop._graphs) == 1
    assert len(calls) == 2 + 1 + 1 + 3      # captured again: warm-up, one iteration, graph_iterations of them
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
