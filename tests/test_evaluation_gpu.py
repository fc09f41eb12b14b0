"""GPU: the synthetic-view evaluation loop (``sdfest_amd.evaluation``): ``generate_views`` against the reference's
dictionary and camera algebra (tests/golden/eval_views.npz), and ``evaluate_mesh`` end to end with the mug decoder --
views of a known latent's mesh -> SDFPipeline -> the estimate's mesh -> samples -> metrics."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN

pytestmark = pytest.mark.gpu

T = lambda a, dt=torch.float32: torch.tensor(np.asarray(a), dtype=dt, device="cuda")


def mug_pipeline(W, H, f, n_iter, init_network=None, **extra):
    from sdfest_amd import SDFPipeline
    from sdfest_amd.synthetic import plausible_init_network_state
    from test_sdfpipeline_gpu import make_config, mug_weights
    cfg = make_config(W, H, f, f, W / 2, H / 2, 0.005, n_iter, **extra)
    if init_network is not None:
        return SDFPipeline(cfg, vae_state_dict=mug_weights(), init_network=init_network)
    return SDFPipeline(cfg, vae_state_dict=mug_weights(), init_state_dict=plausible_init_network_state())


def mug_latents():
    return np.load(os.path.join(GOLDEN, "decoder_mug.npz"))["z"]


def test_generate_views_dictionary_masks_and_golden_poses():
    from sdfest_amd import render_mesh_depth
    from sdfest_amd.evaluation import generate_views
    pipe = mug_pipeline(160, 120, 150.0, 2, iso_threshold=0.0)
    mesh = pipe.generate_mesh(T(mug_latents()[9:10]) * 0.5, T([0.055]), True)
    mesh.position = T([0.3, 0.2, 0.1])             # set to zero by generate_views, as the reference does
    V, H, W = 5, 120, 160
    views = generate_views(mesh, pipe.cam, V, 0.5, torch.Generator().manual_seed(4))
    assert sorted(views) == ["camera_orientations", "camera_positions", "color_images", "depth_images", "masks"]
    assert tuple(views["depth_images"].shape) == (V, H, W) and views["depth_images"].dtype == torch.float32
    assert tuple(views["masks"].shape) == (V, H, W) and views["masks"].dtype == torch.bool
    assert tuple(views["color_images"].shape) == (V, H, W, 3) and not views["color_images"].any()
    assert tuple(views["camera_positions"].shape) == (V, 3) and tuple(views["camera_orientations"].shape) == (V, 4)
    assert all(t.is_cuda for t in views.values())
    assert torch.equal(views["masks"], views["depth_images"] != 0)
    assert views["masks"].flatten(1).sum(1).min().item() > 100
    assert not mesh.position.any()
    assert torch.allclose(views["camera_positions"].norm(dim=1), torch.full((V,), 0.5, device="cuda"), atol=1e-6)
    assert torch.allclose(views["camera_orientations"].norm(dim=1), torch.ones(V, device="cuda"), atol=1e-6)
    # the same generator state: the same views
    again = generate_views(mesh, pipe.cam, V, 0.5, torch.Generator().manual_seed(4))
    assert all(torch.equal(views[k], again[k]) for k in views)
    # the golden algebra: the reference's lines with the reference's quaternion functions
    g = np.load(os.path.join(GOLDEN, "eval_views.npz"))
    for i in range(len(g["camera_distances"])):
        dist = float(g["camera_distances"][i])
        mesh.orientation = T(g["mesh_orientations"][i])
        got = generate_views(mesh, pipe.cam, 1, dist, camera_orientations=T(g["camera_orientations"][i:i + 1]))
        assert np.allclose(got["camera_positions"].cpu().numpy()[0], g["camera_positions"][i], atol=1e-6)
        want = render_mesh_depth(mesh, pipe.cam, T([[0.0, 0.0, dist]]), T(g["mesh_orientations_cam"][i:i + 1]),
                                 convention="open3d")
        a, b = got["depth_images"][0], want[0]
        assert (b > 0).sum() > 50
        # float32 algebra on the device against the golden's float64: the pose differs in the last bits
        assert ((a > 0) != (b > 0)).float().mean().item() < 1e-3
        both = (a > 0) & (b > 0)
        assert (a[both] / b[both] - 1).abs().median().item() < 1e-6
        assert ((a[both] / b[both] - 1).abs() > 1e-4).float().mean().item() < 5e-3
    with pytest.raises(ValueError, match="see nothing"):
        generate_views(mesh, pipe.cam, 1, -0.5, camera_orientations=T([[0, 0, 0, 1.0]]))     # the mesh behind the camera


def test_views_feed_the_pipeline_with_the_real_initialisation_network():
    """the dictionary goes into SDFPipeline.__call__ as it is; all metrics finite"""
    from sdfest_amd.evaluation import DEFAULT_METRICS, evaluate_mesh, evaluate_meshes
    pipe = mug_pipeline(160, 120, 150.0, 10, iso_threshold=0.0)
    lat = mug_latents()
    meshes = []
    for i, s in ((9, 0.055), (10, 0.06)):
        m = pipe.generate_mesh(T(lat[i:i + 1]) * 0.5, T([s]), True)
        m.orientation = T([0.2, 0.6, -0.15, 0.75]) / float(np.linalg.norm([0.2, 0.6, -0.15, 0.75]))
        meshes.append(m)
    metrics = evaluate_mesh(pipe, meshes[0], 2, 0.5, 5000, 0, generator=torch.Generator().manual_seed(1))
    assert sorted(metrics) == sorted(DEFAULT_METRICS)
    assert all(np.isfinite(v) for v in metrics.values()), metrics
    assert 0 < metrics["chamfer"] < 0.1 and 0 <= metrics["accuracy_0_01"] <= 1
    stats = evaluate_meshes(pipe, meshes, 2, 0.5, 5000, 0, generator=torch.Generator().manual_seed(1))
    assert sorted(stats) == sorted(DEFAULT_METRICS)
    for name, st in stats.items():
        assert sorted(st) == ["mean", "std", "var"] and all(np.isfinite(v) for v in st.values())
        assert st["var"] >= 0 and st["std"] == pytest.approx(st["var"] ** 0.5)


def test_evaluate_mesh_improves_on_its_initialisation():
    """The scene of tests/test_pipeline_gpu.py::test_c5_full_loop_converges (mug config, 640 x 480, 50 iterations,
    shape optimisation on, latent z[9] / 2, orientation (0.2, 0.6, -0.15, 0.75), scale 0.055, the camera 0.5 away, the
    start 0.01 off in every coordinate, (0.06, -0.05, 0.04, 0) off in orientation, scale 0.06, latent 0) -- but the
    observation comes from the TRIANGLES of the true shape's mesh, through the rasteriser, not from the sphere tracer
    the loop inverts; the true pose is the world's (the mesh at the origin), the cameras are generate_views'.  The
    estimate improves on the start in that test's sense (position error below 0.6 of the start's, scale closer), and
    in the metrics' (a smaller chamfer distance than the start's mesh)."""
    from sdfest_amd import evaluate_metrics, sample_points
    from sdfest_amd.evaluation import DEFAULT_METRICS, evaluate_mesh
    z_true = T(mug_latents()[9:10]) * 0.5
    q_true = T([[0.2, 0.6, -0.15, 0.75]])
    q_true = q_true / q_true.norm()
    p_true = torch.zeros((1, 3), device="cuda")
    p0 = p_true + T([[0.01, 0.01, 0.01]])
    q0 = q_true + T([[0.06, -0.05, 0.04, 0.0]])
    q0 = q0 / q0.norm()
    s0, z0 = T([0.06]), torch.zeros((1, 8), device="cuda")
    start = lambda depth_images, cam_pos, cam_quat, prior, train_prior: (z0.clone(), p0.clone(), s0.clone(), q0.clone())
    pipe = mug_pipeline(640, 480, 320.0, 50, init_network=start, iso_threshold=0.0)
    gt = pipe.generate_mesh(z_true, T([0.055]), True)
    gt.orientation = q_true[0]
    metrics, details = evaluate_mesh(pipe, gt, 2, 0.5, 20000, 0, generator=torch.Generator().manual_seed(0),
                                     return_details=True)
    assert sorted(metrics) == sorted(DEFAULT_METRICS) and all(np.isfinite(v) for v in metrics.values()), metrics
    assert details["views"]["masks"].flatten(1).sum(1).min().item() > 2000
    position, orientation, scale, latent = details["estimate"]
    pos_err0, pos_err = (p0 - p_true).norm().item(), (position - p_true).norm().item()
    start_mesh = pipe.generate_mesh(z0, s0, True)
    start_mesh.position, start_mesh.orientation = p0[0], q0[0]
    start_metrics = evaluate_metrics(details["gt_points"], sample_points([start_mesh], 20000, 0)[0], DEFAULT_METRICS)
    print(f"position error {pos_err0:.4f} -> {pos_err:.4f}; scale 0.06 -> {scale.item():.4f} (true 0.055); chamfer "
          f"{start_metrics['chamfer']:.5f} -> {metrics['chamfer']:.5f}; metrics {metrics}")
    assert pos_err < 0.6 * pos_err0, (pos_err0, pos_err)
    assert abs(scale.item() - 0.055) < abs(0.06 - 0.055)
    assert latent.abs().max().item() > 1e-3          # the latent really was optimised
    assert metrics["chamfer"] < start_metrics["chamfer"]
