"""GPU: ``SDFPipeline.pose_uncertainty`` -- after ``__call__`` on G7 run C's two views (the small configuration of
tests/test_sdfpipeline_gpu.py) against the float64 twin fed the pipeline's own final estimate, and after
``estimate_objects`` with K = 2 objects seen from V = 2 cameras (the scene of tests/test_multi_object_views_gpu.py)."""
import numpy as np
import pytest
import torch

import information_twin as twin
from test_multi_object_views_gpu import F, H, W, scene  # noqa: F401  (the module-scoped scene fixture)
from test_render_gpu import REL
from test_sdfpipeline_gpu import T, g7, make_config, mug_weights, plausible_init_state  # noqa: F401  (g7: a fixture)

pytestmark = pytest.mark.gpu


def g7_pipeline(g7, **extra):
    from sdfest_amd import SDFPipeline
    cfg = make_config(int(g7["c_W"]), int(g7["c_H"]), float(g7["c_fx"]), float(g7["c_fy"]), float(g7["c_cx"]),
                      float(g7["c_cy"]), float(g7["thr"]), 12, far_field=50.0, **extra)
    init = g7["c_init"]
    fixed_init = lambda *a: (T(init[None, 8:]), T(init[None, 0:3]), T(init[7:8]), T(init[None, 3:7]))
    pipe = SDFPipeline(cfg, vae_state_dict=mug_weights(), init_network=fixed_init)
    depth = T(g7["c_depth_images"])
    args = (torch.ones_like(depth, dtype=torch.bool), torch.zeros(depth.shape + (3,), device="cuda"))
    kw = dict(camera_positions=T(g7["c_cam_pos"]), camera_orientations=T(g7["c_cam_quat"]), shape_optimization=False)
    return pipe, lambda: pipe(depth.clone(), *args, **kw)


def twin_information(pipe, thr=0.0):
    """(H7 (K,7,7), bound (K,7,7), rss (K,), count (K,)) of the views pose_uncertainty looks at, from the float64 oracle:
    each view's Gram matrix and its yardstick sum |f_i f_j| pushed through T (the yardstick through |T|)."""
    v = pipe._uncertainty_views()
    K, V = v["K"], v["V"]
    fx, fy, cx, cy, _ = pipe.cam.get_pinhole_camera_parameters(0.5)
    n = lambda t: t.detach().cpu().numpy()
    H7, bound, rss, cnt = np.zeros((K, 7, 7)), np.zeros((K, 7, 7)), np.zeros(K), np.zeros(K)
    for i in range(K * V):
        sdf = n(v["sdf"]) if v["sdf"].dim() == 3 else n(v["sdf"][i])
        depth, target = n(v["depth"][i]), n(v["target"][i])
        p, q, s = n(v["position"][i]).astype(np.float64), n(v["orientation"][i]).astype(np.float64), float(v["inv_scale"][i])
        f = twin.features(depth, target, sdf, p, q, s, cx, cy, fx, fy)
        g, yard = twin.gram(f, twin.included(depth, target, thr))
        Tm = twin.tangent_map(q, s, n(v["camera_orientations"][i]).astype(np.float64))
        H7[i // V] += twin.tangent_information(g, q, s, n(v["camera_orientations"][i]).astype(np.float64))
        bound[i // V] += np.abs(Tm).T @ yard[:8, :8] @ np.abs(Tm)
        rss[i // V] += g[8, 8]
        cnt[i // V] += g[9, 9]
    return H7, bound, rss, cnt


def test_needs_an_estimate(g7):
    pipe, _ = g7_pipeline(g7)
    with pytest.raises(RuntimeError, match="needs an estimate"):
        pipe.pose_uncertainty()


def test_after_call_matches_the_twin_at_the_final_estimate(g7):
    pipe, run = g7_pipeline(g7)
    run()
    for thr_arg, thr in ((None, 0.0), (True, 0.03)):
        rec = pipe.pose_uncertainty(inlier_threshold=thr_arg)
        assert rec.information.shape == (1, 7, 7) and rec.covariance.shape == (1, 7, 7) and rec.rank.shape == (1,)
        assert rec.position_std.shape == (1, 3) and rec.rotation_std_deg.shape == (1, 3) and rec.scale_rel_std.shape == (1,)
        cov = rec.covariance[0].cpu().numpy()
        w = np.linalg.eigvalsh(cov)
        assert np.array_equal(cov, cov.T) and w.min() >= -1e-9 * w.max()
        H7, bound, rss, cnt = twin_information(pipe, thr)
        assert cnt[0] > 100
        err = np.abs(rec.information[0].cpu().numpy() - H7[0])
        print(f"threshold {thr}: {int(cnt[0])} pixels, information at {np.max(err / bound[0]):.3e} of the bound's yardstick")
        assert np.all(err <= REL * bound[0])
        t = twin.pose_covariance(H7[0], rss[0], cnt[0], 1e-6)
        assert int(rec.rank[0]) == t["rank"]
        assert abs(float(rec.sigma2[0]) - t["sigma2"]) <= 1e-4 * t["sigma2"]
    assert thr == 0.03 and cnt[0] < twin_information(pipe)[3][0]      # the pipeline's threshold does cut into the overlap


def test_after_estimate_objects_views_add_in_the_world_tangent(scene):  # noqa: F811
    from sdfest_amd import SDFPipeline, render_information, tangent_information
    K, V = 2, 2
    frames, masks = scene["frames"], scene["masks"][:K].contiguous()
    cfg = make_config(W, H, F, F, W / 2, H / 2, 0.005, 4, far_field=2.0)
    pipe = SDFPipeline(cfg, vae_state_dict=mug_weights(), init_state_dict=plausible_init_state())
    pipe.estimate_objects(frames, masks, scene["cam_pos"], scene["cam_quat"], shape_optimization=False)
    rec = pipe.pose_uncertainty()
    assert rec.information.shape == (K, 7, 7) and rec.rank.shape == (K,)
    v = pipe._uncertainty_views()
    assert (v["K"], v["V"]) == (K, V) and torch.equal(v["camera_orientations"], scene["cam_quat"].repeat(K, 1))
    gram = render_information(v["depth"], v["target"], v["sdf"], v["position"], v["orientation"], v["inv_scale"], pipe.cam)
    print('included pixels per view:', gram[:, 9, 9].tolist())
    assert (gram[:, 9, 9] >= 20).all()
    for k in range(K):
        total = sum(tangent_information(gram[i:i + 1], v["orientation"][i:i + 1], v["inv_scale"][i:i + 1],
                                        v["camera_orientations"][i:i + 1])[0] for i in range(k * V, (k + 1) * V))
        assert (rec.information[k] - total).abs().max() <= 1e-12 * total.abs().max()
    # in the camera frame the two views would NOT add to this: the second camera is turned by 20 degrees
    camera_frame = sum(tangent_information(gram[i:i + 1], v["orientation"][i:i + 1], v["inv_scale"][i:i + 1])[0] for i in range(V))
    assert (rec.information[0] - camera_frame).abs().max() > 1e-3 * camera_frame.abs().max()
    # the other object's observation replaced (by nothing): row 0 keeps its bits, row 1 reports an empty overlap
    pipe._last_multi_loop.target.view(K, V, H, W)[1].zero_()
    rec2 = pipe.pose_uncertainty()
    assert torch.equal(rec2.information[0], rec.information[0]) and torch.equal(rec2.sigma2[0], rec.sigma2[0])
    assert torch.allclose(rec2.covariance[0], rec.covariance[0], rtol=1e-12, atol=0) and rec2.rank[0] == rec.rank[0]
    assert int(rec2.rank[1]) == 0 and not rec2.information[1].any() and torch.isnan(rec2.sigma2[1])


def test_a_following_call_returns_what_it_returned_before(g7):
    pipe, run = g7_pipeline(g7)
    run()
    before = [t.clone() for t in run()]
    rec = pipe.pose_uncertainty(inlier_threshold=True)
    assert int(rec.rank[0]) >= 1
    after = run()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
