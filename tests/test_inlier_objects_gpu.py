"""GPU, C ABI: sdfr_inlier_ratio_objects -- the inlier bookkeeping of simple_setup.py:177-211 for K objects in two
launches -- against K calls of the single-object sdfr_inlier_ratio (bit for bit) and a float64 numpy twin.

Every valid pixel's relative error |in - est| / in is generated at least 1e-3 away from the threshold: float32 forms it
to ~2e-7 of that, so the twin, the single-object kernel and the K-object kernel cannot disagree about a pixel, the
counts are integers, and every comparison below is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

THR = 0.03
K, NP = 3, 11
# (W, H): 48 x 32 = 1536 pixels, two 1024-pixel chunks with the second partial, rows on 16-byte boundaries;
# 33 x 25 = 825 pixels, no multiple of 64 or of 4: objects 1 and 2 start off the boundary
SHAPES = [(48, 32), (33, 25)]
SHARE = (0.3, 0.6, 0.4)      # object 0's share of inliers in the three calls: up, then down


def scene(W, H, seed):
    """inputs [K][H][W] and the three calls' estimates [3][K][H][W].  Object 0: a fifth of the pixels without input
    depth, SHARE[c] of the rest inliers; object 1: every pixel valid and an inlier; object 2: no valid pixel."""
    rng = np.random.default_rng(seed)
    n = W * H
    din = rng.uniform(0.5, 2.0, (K, n)).astype(np.float32)
    din[0, rng.random(n) < 0.2] = 0.0
    din[2] = 0.0
    est = np.zeros((3, K, n), np.float32)
    for c in range(3):
        inl = rng.random(n) < SHARE[c]
        r = np.where(inl, rng.uniform(0.0, THR - 1e-3, n), rng.uniform(THR + 1e-3, 0.5, n)) * rng.choice([-1.0, 1.0], n)
        est[c, 0] = (din[0].astype(np.float64) * (1.0 + r)).astype(np.float32)
        est[c, 0, rng.random(n) < 0.1] = 0.0                       # rays that missed: relative error 1, or 0 / 0
        est[c, 1] = (din[1].astype(np.float64) * (1.0 + rng.uniform(-(THR - 1e-3), THR - 1e-3, n))).astype(np.float32)
        est[c, 2] = rng.uniform(0.0, 2.0, n).astype(np.float32) * (rng.random(n) < 0.7)      # x / 0 = inf, 0 / 0 = NaN
    # the generator's promise, as the kernels will see the numbers
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(din[None].astype(np.float64) - est) / din[None]
    valid = np.broadcast_to(din[None] != 0, rel.shape)
    assert np.all(np.abs(rel[valid] - THR) >= 0.99e-3)
    return din.reshape(K, H, W), est.reshape(3, K, H, W)


def twin(din, est):
    """(ratio float32, inliers, valid) of one image pair, in float64"""
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(din.astype(np.float64) - est.astype(np.float64)) / din.astype(np.float64)
        inl, val = int(np.count_nonzero(rel < THR)), int(np.count_nonzero(din))
        return np.float32(inl) / np.float32(val), inl, val


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def runs(request):
    """the three calls through both entry points, everything read back once"""
    from sdfest_amd import _lib
    L = _lib.lib()
    W, H = request.param
    din_np, est_np = scene(W, H, seed=W)
    dev = torch.device("cuda")
    cu = lambda a, dt=torch.float32: torch.tensor(a, dtype=dt, device=dev)
    din = cu(din_np)
    rng = np.random.default_rng(7)
    params_np = rng.normal(size=(3, K, NP)).astype(np.float32)
    MH = 4
    st = torch.cuda.current_stream().cuda_stream

    def fresh(max_history):
        return dict(counts=torch.zeros((K, 2), dtype=torch.int32, device=dev),
                    # one word more than [K][max_history]: the guard behind the history
                    history=torch.cat([torch.full((K * max_history,), -7.0, device=dev), cu([12345.0])]),
                    state=torch.zeros((K, 3), device=dev), best=torch.full((K, NP), -1.0, device=dev))

    objs, strided, short = fresh(MH), fresh(MH), fresh(2)
    single = [dict(counts=torch.zeros(2, dtype=torch.int32, device=dev), history=torch.full((MH,), -7.0, device=dev),
                   state=torch.zeros(3, device=dev), best=torch.full((NP,), -1.0, device=dev)) for _ in range(K)]
    seen = {"objs": [], "strided": [], "short": [], "single": []}
    snap = lambda b: {k: v.clone() for k, v in b.items()}
    for c in range(3):
        step = torch.full((K,), c + 1, dtype=torch.int32, device=dev)
        params = cu(params_np[c])
        est = cu(est_np[c])
        # [K][2][H][W] with the first views poisoned: only the last view of each object may be read
        two = torch.stack([torch.full_like(est, float("nan")), est], dim=1).contiguous()
        for b, e, stride, mh in ((objs, est, W * H, MH), (strided, two[:, 1], 2 * W * H, MH), (short, est, W * H, 2)):
            ptr = e.data_ptr() if e is est else two.data_ptr() + 4 * W * H
            _lib.check(L.sdfr_inlier_ratio_objects(din.data_ptr(), ptr, stride, K, W, H, THR, step.data_ptr(),
                                                   b["counts"].data_ptr(), b["history"].data_ptr(), mh,
                                                   b["state"].data_ptr(), params.data_ptr(), NP, b["best"].data_ptr(),
                                                   0, st), "sdfr_inlier_ratio_objects")
        for k in range(K):
            b = single[k]
            _lib.check(L.sdfr_inlier_ratio(din[k].data_ptr(), est[k].data_ptr(), W, H, THR, step[k:].data_ptr(),
                                           b["counts"].data_ptr(), b["history"].data_ptr(), MH, b["state"].data_ptr(),
                                           params[k].data_ptr(), NP, b["best"].data_ptr(), 0, st), "sdfr_inlier_ratio")
        torch.cuda.synchronize()
        seen["objs"].append(snap(objs)); seen["strided"].append(snap(strided)); seen["short"].append(snap(short))
        seen["single"].append([snap(b) for b in single])
    ratios = np.array([[twin(din_np[k], est_np[c, k])[0] for k in range(K)] for c in range(3)], np.float32)
    counts = [[twin(din_np[k], est_np[c, k])[1:] for k in range(K)] for c in range(3)]
    return dict(seen=seen, ratios=ratios, counts=counts, params=params_np, MH=MH)


def test_equals_k_single_calls_bit_for_bit(runs):
    MH = runs["MH"]
    for c in range(3):
        got = runs["seen"]["objs"][c]
        for k in range(K):
            ref = runs["seen"]["single"][c][k]
            assert torch.equal(bits(got["history"][k * MH:(k + 1) * MH]), bits(ref["history"])), (c, k)
            assert torch.equal(bits(got["state"][k]), bits(ref["state"])), (c, k)
            assert torch.equal(bits(got["best"][k]), bits(ref["best"])), (c, k)
        assert not got["counts"].any()          # left zero for the next call ...
        assert got["history"][-1].item() == 12345.0


def test_equals_the_float64_twin(runs):
    MH, ratios = runs["MH"], runs["ratios"]
    # the scene does what it says: object 0 up then down, object 1 all inliers, object 2 nothing valid
    assert ratios[0, 0] < ratios[2, 0] < ratios[1, 0]
    assert np.all(ratios[:, 1] == 1.0) and np.all(np.isnan(ratios[:, 2]))
    assert all(runs["counts"][c][2] == (0, 0) for c in range(3)) and runs["counts"][0][0][1] > 0
    for c in range(3):
        got = runs["seen"]["objs"][c]
        hist = got["history"][:K * MH].view(K, MH).cpu().numpy()
        for k in range(K):
            assert np.array_equal(hist[k, :c + 1].view(np.int32), ratios[:c + 1, k].view(np.int32)), (c, k)
            assert np.all(hist[k, c + 1:] == -7.0)          # nothing written ahead of the step
    last = runs["seen"]["objs"][2]
    state, best = last["state"].cpu().numpy(), last["best"].cpu().numpy()
    # object 0: the best is iteration 2, with the parameters of that call
    assert state[0].tolist() == [float(ratios[1, 0]), 2.0, 1.0] and np.array_equal(best[0], runs["params"][1, 0])
    # object 1: 1.0 three times -- ties do not win, iteration 1 stays
    assert state[1].tolist() == [1.0, 1.0, 1.0] and np.array_equal(best[1], runs["params"][0, 1])
    # object 2: NaN at iteration 1 (the first counts), and nothing is greater than NaN
    assert np.isnan(state[2, 0]) and state[2, 1:].tolist() == [1.0, 1.0] and np.array_equal(best[2], runs["params"][0, 2])


def test_object_stride_reads_the_last_view_only(runs):
    for c in range(3):
        a, b = runs["seen"]["objs"][c], runs["seen"]["strided"][c]
        for name in ("history", "state", "best", "counts"):
            assert torch.equal(bits(a[name]), bits(b[name])), (c, name)


def test_history_is_written_inside_its_bounds_only(runs):
    """max_history = 2: the third ratio goes nowhere -- not into the next object's row, not behind the buffer"""
    ratios = runs["ratios"]
    for c in range(3):
        got = runs["seen"]["short"][c]
        hist = got["history"][:K * 2].view(K, 2).cpu().numpy()
        n = min(c + 1, 2)
        for k in range(K):
            assert np.array_equal(hist[k, :n].view(np.int32), ratios[:n, k].view(np.int32)), (c, k)
            assert np.all(hist[k, n:] == -7.0)
        assert got["history"][-1].item() == 12345.0          # the guard word behind the history
        assert not got["counts"].any()
        # the rest of the bookkeeping does not depend on the history's length
        full = runs["seen"]["objs"][c]
        assert torch.equal(bits(got["state"]), bits(full["state"])) and torch.equal(bits(got["best"]), bits(full["best"]))
