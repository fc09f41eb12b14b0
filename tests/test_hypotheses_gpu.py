"""GPU: N orientation hypotheses of one object -- the N most probable cells of the initialisation network's posterior
(``sdfr_orientation_topk``), N starts of the loop from them (``sdfr_init_hypotheses``), refined side by side as N rows of
``MultiObjectRenderAndCompare`` and the best supported one selected on the device (``sdfr_select_row``) -- through
``SDFPoseNet.orientation_topk``, ``ResidentInit(hypotheses=N)``, ``SDFPipeline.refine_hypotheses`` /
``estimate_hypotheses`` / ``last_hypotheses`` and the config key ``orientation_hypotheses``.  The kernels are compared
bit for bit with the numpy statements of their rules (tests/hypotheses_twin.py)."""
import os

import numpy as np
import pytest
import torch

import hypotheses_twin as twin
from helpers import GOLDEN
from test_sdfpipeline_gpu import make_config, mug_weights, plausible_init_state

pytestmark = pytest.mark.gpu

T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device="cuda")
bits = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a.cpu().numpy() if torch.is_tensor(a) else a), bits(b.cpu().numpy() if torch.is_tensor(b) else b))


def geodesic(q, p):
    q, p = np.asarray(q, dtype=np.float64).ravel(), np.asarray(p, dtype=np.float64).ravel()
    return 2.0 * np.arccos(np.clip(abs(np.dot(q, p)) / (np.linalg.norm(q) * np.linalg.norm(p)), 0.0, 1.0))


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


@pytest.fixture(scope="module")
def net():
    from sdfest_amd.init_network import SDFPoseNet
    from sdfest_amd.synthetic import MUG_INIT_BACKBONE, MUG_INIT_HEAD, init_network_state
    return SDFPoseNet(MUG_INIT_BACKBONE, MUG_INIT_HEAD, 8, init_network_state(3))


# ---- 1. sdfr_orientation_topk -------------------------------------------------------------------------------------
def posteriors(C, rng):
    """name -> (C,) float32: the seeded inputs of the issue"""
    p = np.exp(rng.normal(size=C)); p = (p / p.sum()).astype(np.float32)
    out = {"softmax": p,
           # 8 levels: many equal values, spread over the threads and waves of the workgroup
           "quantised": (np.floor(p / p.max() * 7.999) / 8).astype(np.float32),
           "equal": np.full(C, 1.0 / C, dtype=np.float32)}
    nan0 = p.copy(); nan0[0] = np.nan
    out["nan_at_0"] = nan0
    last = p.copy(); last[C - 1] = 2.0
    out["max_at_end"] = last
    return out


@pytest.mark.parametrize("C", [1, 5, 63, 64, 65, 255, 256, 257, 576, 4608, 36864])
def test_topk_against_the_twin(net, C):
    rng = np.random.default_rng(100 + C)
    for name, p in posteriors(C, rng).items():
        for N in (1, 2, 5, 32):
            if N > C:
                continue
            idx, prob = net.orientation_topk(T(p), N)
            want_idx, want_prob = twin.topk(p, N)
            assert idx.dtype == torch.int32 and idx.cpu().numpy().tolist() == want_idx.tolist(), (name, C, N)
            assert same_bits(prob, want_prob), (name, C, N)
            if name == "equal":
                assert want_idx.tolist() == list(range(N))
    if C >= 5:      # three non-zero entries, five asked for: the zeros fill in index order
        p = np.zeros(C, dtype=np.float32)
        where = rng.choice(C, 3, replace=False)
        p[where] = [0.2, 0.5, 0.3]
        idx, prob = net.orientation_topk(T(p), 5)
        zeros = [i for i in range(C) if i not in where][:2]
        assert idx.cpu().numpy().tolist() == [int(where[1]), int(where[2]), int(where[0])] + zeros
        assert idx.cpu().numpy().tolist() == twin.topk(p, 5)[0].tolist() and same_bits(prob, twin.topk(p, 5)[1])


@pytest.mark.parametrize("C", [5, 576, 4608])
def test_topk_entry_0_is_the_posterior_kernels_argmax(net, C):
    rng = np.random.default_rng(7 + C)
    logits = T(rng.normal(size=C) * 2.0)
    prior = rng.uniform(0.0, 1.0, C); prior[rng.choice(C, C // 3, replace=False)] = 0.0
    train = rng.uniform(0.5, 1.5, C)
    for pr, tp in ((None, None), (T(prior / prior.sum()), None), (T(prior / prior.sum()), T(train / train.sum()))):
        post, index, maximum = net.orientation_posterior(logits, pr, tp)
        idx, prob = net.orientation_topk(post, min(C, 4))
        assert int(idx[0]) == int(index[0]) and same_bits(prob[0:1], maximum)
        assert idx.cpu().numpy().tolist() == twin.topk(post.cpu().numpy(), min(C, 4))[0].tolist()


def test_topk_refuses_what_the_header_excludes(net):
    for n in (0, 33, 6):
        with pytest.raises(RuntimeError, match="sdfr_orientation_topk"):
            net.orientation_topk(torch.zeros(5, device="cuda"), n)


# ---- 2. sdfr_init_hypotheses --------------------------------------------------------------------------------------
def test_init_hypotheses_rows(net):
    from sdfest_amd import _lib
    from sdfest_amd.init_network import grid_quat_table
    L = _lib.lib()
    rng = np.random.default_rng(11)
    C, sd = net.grid.num_cells(), 8
    grid = grid_quat_table(net.grid, net.dev)
    head = T(rng.normal(size=sd + 4 + C))
    cam_quat = rng.normal(size=4); cam_quat /= np.linalg.norm(cam_quat)
    cam_quat, cam_pos, centroid = T(cam_quat), T([0.1, -0.2, 0.3]), T([0.01, 0.02, -0.5])
    post, index, maximum = net.orientation_posterior(head[sd + 4:])
    one = torch.zeros(8 + sd, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.sdfr_init_estimate(head.data_ptr(), sd, grid.data_ptr(), index.data_ptr(), centroid.data_ptr(),
                                    cam_pos.data_ptr(), cam_quat.data_ptr(), 0, 0, None, None, one.data_ptr(), 0, st),
               "sdfr_init_estimate")
    N = 7
    # the argmax first, then random cells, one of them twice, and two outside the table (clamped on the device)
    idx = np.array([int(index[0])] + rng.integers(0, C, 3).tolist() + [C + 40, -3, int(index[0])], dtype=np.int32)
    rows = torch.full((N, 8 + sd), -7.0, device="cuda")
    idx_d = torch.tensor(idx, device="cuda")
    _lib.check(L.sdfr_init_hypotheses(one.data_ptr(), 8 + sd, grid.data_ptr(), C, idx_d.data_ptr(), N,
                                      cam_quat.data_ptr(), rows.data_ptr(), 0, st), "sdfr_init_hypotheses")
    got, one_h = rows.cpu().numpy(), one.cpu().numpy()
    for j in range(N):      # position, scale and latent: params_one's bits
        assert same_bits(got[j, :3], one_h[:3]) and same_bits(got[j, 7:], one_h[7:])
    assert same_bits(got[0, 3:7], one_h[3:7]) and same_bits(got[6], one_h)        # the argmax's row IS sdfr_init_estimate's
    want = twin.init_hypotheses(one_h, grid.cpu().numpy(), idx, cam_quat.cpu().numpy())
    assert same_bits(got, want)
    assert same_bits(got[4, 3:7], twin.quat_mul_world(cam_quat.cpu().numpy(), grid.cpu().numpy()[C - 1]))
    assert same_bits(got[5, 3:7], twin.quat_mul_world(cam_quat.cpu().numpy(), grid.cpu().numpy()[0]))
    # ... and the product is the quaternion product: against float64, 4 half-ulps of |a| |b| (tests/test_hypotheses_cpu.py)
    ref = qmul(cam_quat.cpu().numpy().astype(np.float64), grid.cpu().numpy()[idx[1]].astype(np.float64))
    assert np.max(np.abs(got[1, 3:7] - ref)) <= 4 * 2.0 ** -24 * 1.0001


# ---- 3. sdfr_select_row -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 31, 32])
@pytest.mark.parametrize("stride", [1, 3])
def test_select_row_against_the_twin(N, stride):
    from sdfest_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(10 * N + stride)
    n = 16
    rows = rng.normal(size=(N, n)).astype(np.float32)
    cases = {"random": rng.uniform(0, 1, N), "ties": np.round(rng.uniform(0, 1, N) * 3) / 3,
             "nans_in_front": np.concatenate([np.full(N // 2, np.nan), rng.uniform(0, 1, N - N // 2)]),
             "all_nan": np.full(N, np.nan), "all_zero": np.zeros(N),
             "best_last": np.concatenate([rng.uniform(0, 0.5, N - 1), [0.9]])}
    st = torch.cuda.current_stream().cuda_stream
    for name, score in cases.items():
        score = score.astype(np.float32)
        padded = np.full((N, stride), 5.0, dtype=np.float32)      # the other columns hold larger numbers
        padded[:, 0] = score
        s_d, r_d = T(padded), T(rows)
        out_row, out_i, out_s = torch.full((n,), -1.0, device="cuda"), torch.full((1,), -1, dtype=torch.int32, device="cuda"), \
            torch.full((1,), -1.0, device="cuda")
        _lib.check(L.sdfr_select_row(s_d.data_ptr(), stride, N, r_d.data_ptr(), n, out_row.data_ptr(), out_i.data_ptr(),
                                     out_s.data_ptr(), 0, st), "sdfr_select_row")
        j, s, r = twin.select_row(score, rows)
        assert int(out_i[0]) == j, (name, N, stride)
        assert same_bits(out_s, np.array([s])) and same_bits(out_row, r), (name, N, stride)
        if name == "all_nan" or name == "all_zero":
            assert j == 0
        if name == "nans_in_front" and N > 1:
            assert j >= N // 2


# ---- the front door ------------------------------------------------------------------------------------------------
def mug_scene(pipe, q_true, p_true=(0.02, -0.01, -0.5), s_true=0.055, z_row=9, z_scale=0.5):
    """one view of a mug-decoder shape at a known pose: (depth (H,W), mask, z_true (1,L))"""
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    z_true = T(d["z"][z_row:z_row + 1]) * z_scale
    with torch.no_grad():
        depth = pipe.generate_depth(T(p_true), T(q_true), T(s_true), z_true)
    return depth.contiguous(), depth > 0, z_true


Q_TRUE = np.array([0.2, 0.6, -0.15, 0.75]) / np.linalg.norm([0.2, 0.6, -0.15, 0.75])


def small_pipeline(**extra):
    from sdfest_amd import SDFPipeline
    cfg = make_config(64, 48, 90.0, 90.0, 32.0, 24.0, 0.005, 6, **extra)
    return SDFPipeline(cfg, vae_state_dict=mug_weights(), init_state_dict=plausible_init_state())


def test_one_hypothesis_is_estimate_objects_bit_for_bit():
    pipe = small_pipeline()
    depth, mask, _ = mug_scene(pipe, Q_TRUE)
    assert mask.sum() > 150
    assert pipe.last_hypotheses() is None
    got = pipe.estimate_hypotheses(depth, mask, hypotheses=1, shape_optimization=False)
    want = pipe.estimate_objects(depth, mask[None], shape_optimization=False)
    assert [tuple(t.shape) for t in got] == [(1, 3), (1, 4), (1,), (1, 8)]
    for a, b in zip(got, want):
        assert torch.equal(a, b.reshape(a.shape))
    # another observation: nothing is built or captured again
    loop = pipe._last_hypotheses["loop"]
    resident = pipe._resident_hypotheses[1]
    graphs = (loop.graph, loop.graph_many, list(resident._graphs.values()))
    depth2, mask2, _ = mug_scene(pipe, Q_TRUE * np.array([1, -1, 1, 1.0]), p_true=(-0.03, 0.02, -0.55))
    got2 = pipe.estimate_hypotheses(depth2, mask2, hypotheses=1, shape_optimization=False)
    loop2 = pipe._last_hypotheses["loop"]
    assert loop2 is loop and (loop.graph, loop.graph_many, list(resident._graphs.values())) == graphs
    assert graphs[0] is not None and len(graphs[2]) == 1 and loop.graph is graphs[0]
    want2 = pipe.estimate_objects(depth2, mask2[None], shape_optimization=False)
    for a, b in zip(got2, want2):
        assert torch.equal(a, b.reshape(a.shape))
    assert not torch.equal(got[0], got2[0])
    lh = pipe.last_hypotheses()
    assert lh["winner"] == 0 and lh["index"].shape == (1,) and lh["final"].shape == (1, 16)


def test_plumbing_of_four_hypotheses():
    from sdfest_amd.init_network import grid_quat_table
    from sdfest_amd.pipeline import MultiObjectRenderAndCompare
    pipe = small_pipeline()
    depth, mask, _ = mug_scene(pipe, Q_TRUE)
    depth = torch.where(mask, depth, torch.full_like(depth, 1.0))       # a wall behind the object: the mask removes it
    before = depth.clone()
    cam_pos = T([0.3, -0.1, 0.2])
    cam_quat = np.array([0.1, -0.3, 0.2, 0.9]); cam_quat = T(cam_quat / np.linalg.norm(cam_quat))
    out = pipe.estimate_hypotheses(depth, mask, hypotheses=4, camera_positions=cam_pos, camera_orientations=cam_quat,
                                   shape_optimization=False)
    lh = pipe.last_hypotheses()
    assert torch.equal(depth, before)                                    # the caller's depth is only read
    initial, final = lh["initial"].cpu().numpy(), lh["final"].cpu().numpy()
    assert initial.shape == final.shape == (4, 16) and lh["index"].shape == lh["probability"].shape == (4,)
    for j in range(1, 4):
        assert same_bits(initial[j, :3], initial[0, :3]) and same_bits(initial[j, 7:], initial[0, 7:])
    index, prob = lh["index"].cpu().numpy(), lh["probability"].cpu().numpy()
    assert len(set(index.tolist())) == 4 and np.all(np.diff(prob) <= 0)
    grid = grid_quat_table(pipe.init_network.grid, pipe._dev).cpu().numpy()
    assert same_bits(initial, twin.init_hypotheses(initial[0], grid, index, cam_quat.cpu().numpy()))
    # the ranking is the posterior's, and its head the argmax the single estimate starts from
    resident = pipe._resident_hypotheses[4]
    assert index.tolist() == twin.topk(resident.posterior.cpu().numpy(), 4)[0].tolist()
    assert int(resident.index[0]) == int(index[0]) and same_bits(resident.params, initial[0])
    # the same four rows through a fresh K-row loop on the same masked image
    fresh = MultiObjectRenderAndCompare(pipe.vae, pipe.cam, pipe.config, 4, shape_optimization=False, track_inliers=True)
    fresh.rebind(depth[None], cam_pos, cam_quat, masks=mask[None, None].expand(4, 1, -1, -1), far_field=pipe._far_field)
    ini = lh["initial"]
    rows = fresh(ini[:, 0:3], ini[:, 3:7], ini[:, 7], ini[:, 8:])
    assert torch.equal(fresh.params, lh["final"])
    ratio = fresh.inlier_history[:, pipe.config["max_iterations"] - 1]
    assert same_bits(ratio, lh["inlier_ratio"]) and np.all(np.isfinite(ratio.cpu().numpy()))
    assert lh["winner"] == int(np.argmax(lh["inlier_ratio"].cpu().numpy())) == twin.select_row(ratio.cpu().numpy(), final)[0]
    w = lh["winner"]
    for t, lo, hi in zip(out, (0, 3, 7, 8), (3, 7, 8, 16)):
        assert same_bits(t.reshape(-1), final[w, lo:hi])
    # ResidentInit(hypotheses=N): one view of one object only; with 1 there is nothing more than before
    from sdfest_amd.init_network import ResidentInit
    for kw in (dict(views=2), dict(views=1, objects=True), dict(views=1, hypotheses=33), dict(views=1, hypotheses=0)):
        with pytest.raises(ValueError, match="hypotheses"):
            ResidentInit(pipe.init_network, pipe.cam, kw.pop("views"), pipe.config, **dict(dict(hypotheses=2), **kw))
    assert not hasattr(ResidentInit(pipe.init_network, pipe.cam, 1, pipe.config), "params_h")
    # best_inlier_ratio: the score is every row's best ratio, and best_estimates() keeps working
    pipe_b = small_pipeline(result_selection_strategy="best_inlier_ratio")
    out_b = pipe_b.estimate_hypotheses(depth, mask, hypotheses=4, camera_positions=cam_pos, camera_orientations=cam_quat,
                                       shape_optimization=False)
    lb = pipe_b.last_hypotheses()
    best = pipe_b.best_estimates()
    assert len(best) == 4 and same_bits(lb["inlier_ratio"], np.array([b[0] for b in best], dtype=np.float32))
    assert lb["winner"] == twin.select_row(lb["inlier_ratio"].cpu().numpy(), final)[0]
    assert torch.equal(lb["final"], lh["final"]) and same_bits(out_b[1].reshape(-1), final[lb["winner"], 3:7])
    assert np.all(lb["inlier_ratio"].cpu().numpy() >= lh["inlier_ratio"].cpu().numpy())


def test_no_iteration_takes_the_first_row():
    pipe = small_pipeline(max_iterations=0)
    depth, mask, _ = mug_scene(pipe, Q_TRUE)
    out = pipe.estimate_hypotheses(depth, mask, hypotheses=3, shape_optimization=False)
    lh = pipe.last_hypotheses()
    assert lh["winner"] == 0 and torch.equal(lh["initial"], lh["final"])
    assert same_bits(out[1].reshape(-1), lh["initial"][0, 3:7])


def test_the_near_truth_hypothesis_is_recovered():
    """One 160x120 view of a mug with its handle in view, four starts at the true position, scale and latent.  The
    decoded shape's axis is the object's z (its slices along z are rings above two solid slices, the bottom) and its
    handle points along -y.  The starts: upside down (half a turn about x), tipped on its side (a quarter turn about y),
    a seeded random orientation, and -- LAST, so that no tie-break can pick it -- the truth perturbed by normal(0, 0.03)
    per component.  Pose only, 30 iterations.  The last row must win and end nearer the truth than every other row.
    Measured on an MI355X: inlier ratios 0.834, 0.741, 0.848 and 0.979; the winner leads the runner-up by 0.130 (the
    body of a mug is a solid of revolution: a wrong orientation still explains most of its pixels; half a turn about y,
    which leaves the handle where it is, reaches 0.927 and was not taken for that reason)."""
    from sdfest_amd import SDFPipeline
    cfg = make_config(160, 120, 200.0, 200.0, 80.0, 60.0, 0.005, 30)
    pipe = SDFPipeline(cfg, vae_state_dict=mug_weights(), init_state_dict=plausible_init_state())
    p_true, s_true = (0.02, -0.01, -0.5), 0.055
    depth, mask, z_true = mug_scene(pipe, Q_TRUE, p_true, s_true)
    assert mask.sum() > 1000
    rng = np.random.default_rng(21)
    r = np.sqrt(0.5)
    q_rand = rng.normal(size=4); q_rand /= np.linalg.norm(q_rand)
    q_near = Q_TRUE + rng.normal(0, 0.03, 4); q_near /= np.linalg.norm(q_near)
    starts = np.stack([qmul(Q_TRUE, [1.0, 0, 0, 0]), qmul(Q_TRUE, [0, r, 0, r]), q_rand, q_near])
    assert all(geodesic(q, Q_TRUE) > 1.0 for q in starts[:3]) and geodesic(q_near, Q_TRUE) < 0.2
    out = pipe.refine_hypotheses(depth, mask, T(np.repeat(np.array([p_true]), 4, 0)), T(starts), T([s_true] * 4),
                                 z_true.repeat(4, 1), shape_optimization=False)
    lh = pipe.last_hypotheses()
    ratios = lh["inlier_ratio"].cpu().numpy()
    print("hypothesis inlier ratios", ratios.tolist(), "margin", float(ratios[3] - np.max(ratios[:3])))
    assert lh["index"] is None and lh["probability"] is None
    assert lh["winner"] == 3
    dist = [geodesic(q, Q_TRUE) for q in lh["final"][:, 3:7].cpu().numpy()]
    assert geodesic(out[1].cpu().numpy(), Q_TRUE) == dist[3] and all(dist[3] < x for x in dist[:3])
    assert torch.equal(out[3], z_true)                                 # pose only: the latent stays


def test_end_to_end_with_a_prior_on_four_cells():
    """The initialisation network's weights are seeded, so its posterior favours an arbitrary cell; a prior that is
    non-zero on four cells only -- the cell of the true orientation and three far from it -- makes those four the
    hypotheses, and the loop's inlier ratio must pick the true one's cell (measured on an MI355X: 0.509 for it, 0.102,
    0.407 and 0.324 for the others).  The config key routes ``__call__`` to the same
    computation (compared pose-only: with shape optimisation d/dSDF is summed with float atomics and two runs differ in
    their last bits, tests/test_sdfpipeline_gpu.py)."""
    from sdfest_amd import SDFPipeline
    from sdfest_amd.synthetic import MUG_INIT_HEAD, init_network_state
    cfg = make_config(160, 120, 160.0, 160.0, 80.0, 60.0, 0.005, 30)
    pipe = SDFPipeline(cfg, vae_state_dict=mug_weights(), init_state_dict=plausible_init_state())
    depth, mask, _ = mug_scene(pipe, Q_TRUE)
    grid = pipe.init_network.grid
    C = grid.num_cells()
    cells = np.stack([grid.index_to_quat(i) for i in range(C)])
    near = int(grid.quat_to_index(Q_TRUE))
    far = [i for i in np.argsort([-geodesic(c, Q_TRUE) for c in cells]) if i != near]
    rng = np.random.default_rng(4)
    support = [near, int(far[0])] + [int(i) for i in rng.choice(far[1:C // 4], 2, replace=False)]
    assert len(set(support)) == 4 and all(geodesic(cells[i], Q_TRUE) > 1.5 for i in support[1:])
    prior = torch.zeros(C, device="cuda")
    prior[support] = 0.25
    out = pipe.estimate_hypotheses(depth, mask, hypotheses=4, prior_orientation_distribution=prior)
    lh = pipe.last_hypotheses()
    index = lh["index"].cpu().numpy().tolist()
    print("cells", index, "near", near, "inlier ratios", lh["inlier_ratio"].cpu().numpy().tolist())
    assert set(index) == set(support)
    assert index[lh["winner"]] == near
    assert [tuple(t.shape) for t in out] == [(1, 3), (1, 4), (1,), (1, 8)]
    # the config key alone: the front door returns the same tuple
    want = pipe.estimate_hypotheses(depth, mask, hypotheses=4, prior_orientation_distribution=prior,
                                    shape_optimization=False)
    routed = SDFPipeline(dict(cfg, orientation_hypotheses=4), vae_state_dict=mug_weights(),
                         init_state_dict=plausible_init_state())
    before = depth.clone()
    got = routed(depth, mask, None, prior_orientation_distribution=prior, shape_optimization=False)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(depth, before) and routed.last_hypotheses()["index"].cpu().numpy().tolist() == index
    with pytest.raises(ValueError, match="point_constraint"):
        routed(depth, mask, None, point_constraint=(T([0, 0, 0]), T([0, 0, 1]), T([0, 0, -0.5])))
    # what the hypotheses need, each refusal naming its key
    with pytest.raises(ValueError, match="hypotheses"):
        pipe.estimate_hypotheses(depth, mask, hypotheses=33)
    with pytest.raises(ValueError, match="hypotheses"):
        pipe.estimate_hypotheses(depth, mask, hypotheses=0)
    with pytest.raises(ValueError, match="init_view"):
        SDFPipeline(dict(cfg, init_view="best"), vae_state_dict=mug_weights(), init_state_dict=plausible_init_state()
                    ).estimate_hypotheses(torch.stack([depth, depth]), torch.stack([mask, mask]), hypotheses=2)
    with pytest.raises(ValueError, match="resident_init"):
        SDFPipeline(cfg, vae_state_dict=mug_weights(), init_state_dict=plausible_init_state(), resident_init=False
                    ).estimate_hypotheses(depth, mask, hypotheses=2)
    with pytest.raises(ValueError, match="init_network"):
        SDFPipeline(cfg, vae_state_dict=mug_weights(), init_network=lambda *a: None).estimate_hypotheses(depth, mask,
                                                                                                      hypotheses=2)
    head = dict(MUG_INIT_HEAD, orientation_repr="quaternion")
    cfg_q = dict(cfg, init=dict(cfg["init"], head=head))
    pipe_q = SDFPipeline(cfg_q, vae_state_dict=mug_weights(), init_state_dict=init_network_state(7, head=head))
    with pytest.raises(ValueError, match="orientation_repr"):
        pipe_q.estimate_hypotheses(depth, mask, hypotheses=2)


def test_an_empty_mask_raises_no_depth_error():
    from sdfest_amd import NoDepthError
    pipe = small_pipeline()
    depth, mask, z_true = mug_scene(pipe, Q_TRUE)
    with pytest.raises(NoDepthError):
        pipe.estimate_hypotheses(depth, torch.zeros_like(mask), hypotheses=2, shape_optimization=False)
    with pytest.raises(NoDepthError):
        pipe.refine_hypotheses(depth, torch.zeros_like(mask), T([[0, 0, -0.5]] * 2), T([[0, 0, 0, 1.0]] * 2), T([0.05] * 2),
                               z_true.repeat(2, 1), shape_optimization=False)
    # ... and the pipeline takes the next observation
    out = pipe.estimate_hypotheses(depth, mask, hypotheses=2, shape_optimization=False)
    assert all(bool(torch.isfinite(t).all()) for t in out)
