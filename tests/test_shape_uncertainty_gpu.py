"""GPU: ``SDFPipeline.shape_uncertainty`` -- after ``__call__`` on G7 run C's two views against the float64 twin fed the
pipeline's own final estimate and the pipeline's own decoder Jacobian (the construction of
tests/test_pose_uncertainty_gpu.py; the Jacobian itself is tests/test_decoder_jvp_gpu.py's subject), and after
``estimate_objects`` with K = 2 objects seen from V = 2 cameras."""
import numpy as np
import pytest
import torch

import information_twin as twin
import shape_information_twin as st
from test_multi_object_views_gpu import F, H, W, scene  # noqa: F401  (the module-scoped scene fixture)
from test_pose_uncertainty_gpu import g7_pipeline
from test_render_gpu import REL
from test_sdfpipeline_gpu import g7, make_config, mug_weights, plausible_init_state  # noqa: F401  (g7: a fixture)

pytestmark = pytest.mark.gpu


def twin_joint_information(pipe, thr=0.0):
    """(H (K,7+T,7+T), bound, rss (K,), count (K,)) of the views shape_uncertainty looks at, from the float64 oracle: each
    view's joint Gram matrix and its yardstick sum |f_i f_j| pushed through the tangent map (the yardstick through |T|)"""
    v = pipe._shape_uncertainty_views()
    K, V, T = v["K"], v["V"], v["T"]
    fx, fy, cx, cy, _ = pipe.cam.get_pinhole_camera_parameters(0.5)
    n = lambda t: t.detach().cpu().numpy()
    Hj, bound, rss, cnt = np.zeros((K, 7 + T, 7 + T)), np.zeros((K, 7 + T, 7 + T)), np.zeros(K), np.zeros(K)
    for i in range(K * V):
        sdf = n(v["sdf"]) if v["sdf"].dim() == 3 else n(v["sdf"][i])
        R = sdf.shape[-1]
        fields = n(v["jac"][i // V])[:, :T].T.reshape(T, R, R, R).astype(np.float64)
        depth, target = n(v["depth"][i]), n(v["target"][i])
        p, q, s = n(v["position"][i]).astype(np.float64), n(v["orientation"][i]).astype(np.float64), float(v["inv_scale"][i])
        cq = n(v["camera_orientations"][i]).astype(np.float64)
        inc = twin.included(depth, target, thr)
        f10 = twin.features(depth, target, sdf, p, q, s, cx, cy, fx, fy)
        f = st.joint_features(f10, st.latent_features(depth, sdf, p, q, s, cx, cy, fx, fy, inc, fields), T)
        g, yard = twin.gram(f, inc)
        M = np.zeros((8 + T, 7 + T))
        M[:8, :7] = twin.tangent_map(q, s, cq)
        M[8:, 7:] = np.eye(T)
        Hj[i // V] += st.joint_tangent_information(g, q, s, cq)
        bound[i // V] += np.abs(M).T @ yard[:8 + T, :8 + T] @ np.abs(M)
        rss[i // V] += g[8 + T, 8 + T]
        cnt[i // V] += g[9 + T, 9 + T]
    return Hj, bound, rss, cnt


def test_needs_an_estimate(g7):
    pipe, _ = g7_pipeline(g7)
    with pytest.raises(RuntimeError, match="needs an estimate"):
        pipe.shape_uncertainty()


def test_after_call_matches_the_twin_at_the_final_estimate(g7):
    from sdfest_amd.uncertainty import shape_pose_covariance
    pipe, run = g7_pipeline(g7)
    run()
    T = pipe.vae.latent_size
    rec = pipe.shape_uncertainty(sdf_std=True)
    n = 7 + T
    assert rec.information.shape == (1, n, n) and rec.covariance.shape == (1, n, n) and rec.rank.shape == (1,)
    assert rec.pose_covariance.shape == (1, 7, 7) and rec.latent_std.shape == (1, T) and rec.unobserved.shape == (1, n, n)
    assert rec.position_std.shape == (1, 3) and rec.rotation_std_deg.shape == (1, 3) and rec.scale_rel_std.shape == (1,)
    Hj, bound, rss, cnt = twin_joint_information(pipe)
    assert cnt[0] > 100
    # J^T J itself: the prior and sigma2 taken off again (latent_prior = 0 keeps J^T J / sigma2)
    raw = pipe.shape_uncertainty(latent_prior=0.0)
    JtJ = (raw.information[0] * raw.sigma2[0]).cpu().numpy()
    err = np.abs(JtJ - Hj[0])
    print(f"{int(cnt[0])} pixels, joint information at {np.max(err / bound[0]):.3e} of the bound's yardstick (bound {REL:.0e})")
    assert np.all(err <= REL * bound[0] * (1 + 1e-9))
    # its pose block is pose_uncertainty's information
    pose = pipe.pose_uncertainty()
    perr = np.abs(JtJ[:7, :7] - pose.information[0].cpu().numpy())
    print(f"pose block against pose_uncertainty at {np.max(perr / bound[0][:7, :7]):.3e} of the yardstick")
    assert np.all(perr <= REL * bound[0][:7, :7])
    # the covariance: symmetric, positive semi-definite, marginal stds at least the conditional ones
    cov = rec.covariance[0].cpu().numpy()
    w = np.linalg.eigvalsh(cov)
    assert np.array_equal(cov, cov.T) and w.min() >= -1e-9 * w.max()
    assert int(rec.rank[0]) >= int(pose.rank[0]) >= 1 and float(rec.sigma2[0]) > 0
    c = rec.conditional
    print("marginal / conditional position std", (rec.position_std / c.position_std).tolist(),
          "scale", (rec.scale_rel_std / c.scale_rel_std).tolist(), "rank", int(rec.rank[0]))
    assert (rec.position_std >= c.position_std).all() and (rec.rotation_std_deg >= c.rotation_std_deg).all()
    assert (rec.scale_rel_std >= c.scale_rel_std).all()
    # the record is the module's algebra on the summed views
    again = shape_pose_covariance(torch.tensor(JtJ)[None], torch.tensor(rss), torch.tensor(cnt))
    assert int(again.rank[0]) == int(rec.rank[0])
    # the per-voxel standard deviation of the decoded volume
    assert rec.sdf_std.shape == (1, 64, 64, 64) and rec.sdf_std.dtype == torch.float32
    assert torch.isfinite(rec.sdf_std).all() and (rec.sdf_std >= 0).all() and rec.sdf_std.max() > 0
    assert raw.sdf_std is None


def test_after_estimate_objects_views_add_and_objects_are_independent(scene):  # noqa: F811
    from sdfest_amd import SDFPipeline, joint_tangent_information, render_information
    K, V = 2, 2
    frames, masks = scene["frames"], scene["masks"][:K].contiguous()
    cfg = make_config(W, H, F, F, W / 2, H / 2, 0.005, 4, far_field=2.0)
    pipe = SDFPipeline(cfg, vae_state_dict=mug_weights(), init_state_dict=plausible_init_state())
    pipe.estimate_objects(frames, masks, scene["cam_pos"], scene["cam_quat"], shape_optimization=False)
    rec = pipe.shape_uncertainty(latent_prior=0.0, depth_sigma=1.0)      # sigma2 = 1: information is J^T J
    v = pipe._shape_uncertainty_views()
    T = v["T"]
    assert (v["K"], v["V"]) == (K, V) and rec.information.shape == (K, 7 + T, 7 + T)
    assert v["jacobian"].shape[0] == K * V and torch.equal(v["jacobian"][1], v["jac"][0]) and torch.equal(v["jacobian"][2], v["jac"][1])
    for k in range(K):
        total = 0
        for i in range(k * V, (k + 1) * V):      # each view alone: its own single-view call
            g = render_information(v["depth"][i:i + 1], v["target"][i:i + 1], v["sdf"][i].contiguous(), v["position"][i:i + 1],
                                   v["orientation"][i:i + 1], v["inv_scale"][i:i + 1], pipe.cam,
                                   jacobian=v["jacobian"][i].contiguous(), tangents=T)
            assert g[0, 9 + T, 9 + T] >= 20
            total = total + joint_tangent_information(g, v["orientation"][i:i + 1], v["inv_scale"][i:i + 1],
                                                      v["camera_orientations"][i:i + 1])[0]
        assert (rec.information[k] - total).abs().max() <= 1e-12 * total.abs().max()
    # the other object's observation replaced (by nothing): row 0 keeps its bits, row 1 reports an empty overlap
    pipe._last_multi_loop.target.view(K, V, H, W)[1].zero_()
    rec2 = pipe.shape_uncertainty(latent_prior=0.0, depth_sigma=1.0)
    assert torch.equal(rec2.information[0], rec.information[0])
    assert torch.allclose(rec2.covariance[0], rec.covariance[0], rtol=1e-12, atol=0) and rec2.rank[0] == rec.rank[0]
    assert int(rec2.rank[1]) == 0 and not rec2.information[1].any()
    free = pipe.shape_uncertainty()
    assert torch.isnan(free.sigma2[1]) and torch.isfinite(free.sigma2[0])


def test_a_following_call_returns_what_it_returned_before(g7):
    pipe, run = g7_pipeline(g7)
    run()
    before = [t.clone() for t in run()]
    rec = pipe.shape_uncertainty(inlier_threshold=True, sdf_std=True)
    assert int(rec.rank[0]) >= 1
    after = run()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
