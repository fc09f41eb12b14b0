"""CPU: the mesh depth rasteriser's twin (tests/raster_twin.py) against closed forms that do not depend on it, the
C ABI's argument errors, ``Mesh.from_file`` and the camera algebra of ``evaluation.generate_views`` -- no GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import raster_twin as rt
from helpers import GOLDEN


def camera(W=64, H=48, fx=70.0, fy=65.0, cx=30.0, cy=25.5):
    from sdfest_amd import Camera
    return Camera(W, H, fx, fy, cx, cy, pixel_center=0.5)


def pixel_rays(cam):
    W, H, fx, fy, cx, cy = rt.camera_params(cam)
    col, row = np.meshgrid(np.arange(W), np.arange(H))
    return (col + 0.5 - cx) / fx, (row + 0.5 - cy) / fy


@pytest.mark.parametrize("a,b,c", [(0.0, 0.0, 0.7), (0.3, -0.2, 0.5), (-0.15, 0.4, 1.3)])
def test_twin_plane_closed_form(a, b, c):
    """a large two-triangle plane z = a x + b y + c (internal frame) has depth c / (1 - a dx - b dy) at every pixel"""
    cam = camera()
    xy = np.array([[-50, -50], [50, -50], [50, 50], [-50, 50]], dtype=np.float64)
    v = np.concatenate([xy, (a * xy[:, :1] + b * xy[:, 1:] + c)], 1)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    depth, face, _ = rt.render_mesh((v, f), cam, (1.0, (0, 0, 0, 1), (0, 0, 0)), convention="open3d")
    dx, dy = pixel_rays(cam)
    want = c / (1 - a * dx - b * dy)
    assert (want > 0).all() and (face >= 0).all()
    assert np.max(np.abs(depth / want - 1)) < 1e-12
    # float32 arithmetic: a few roundings
    d32 = rt.render_mesh((v, f), cam, (1.0, (0, 0, 0, 1), (0, 0, 0)), convention="open3d", dtype=np.float32)[0]
    assert d32.dtype == np.float32 and np.max(np.abs(d32 / want - 1)) < 2e-6


def test_twin_single_triangle_mask_is_the_half_plane_test():
    cam = camera()
    W, H, fx, fy, cx, cy = rt.camera_params(cam)
    v = np.array([[-0.21, -0.13, 0.9], [0.27, -0.05, 1.4], [0.02, 0.24, 0.7]])
    for f in ([[0, 1, 2]], [[2, 1, 0]]):      # both windings: both faces count
        depth, face, _ = rt.render_mesh((v, np.array(f)), cam, (1.0, (0, 0, 0, 1), (0, 0, 0)), convention="open3d")
        u = fx * v[:, 0] / v[:, 2] + cx - 0.5     # projected vertices in pixel-index coordinates
        w = fy * v[:, 1] / v[:, 2] + cy - 0.5
        col, row = np.meshgrid(np.arange(W), np.arange(H))
        side = [(u[j] - u[i]) * (row - w[i]) - (w[j] - w[i]) * (col - u[i]) for i, j in ((0, 1), (1, 2), (2, 0))]
        inside = ((side[0] >= 0) & (side[1] >= 0) & (side[2] >= 0)) | ((side[0] <= 0) & (side[1] <= 0) & (side[2] <= 0))
        margin = np.min(np.abs(side), 0) > 1e-9
        assert 100 < inside.sum() < W * H // 2
        assert np.array_equal((depth > 0)[margin], inside[margin])
        assert ((face == 0) == (depth > 0)).all()
        assert v[:, 2].min() <= depth[depth > 0].min() and depth.max() <= v[:, 2].max()


def test_twin_conventions_agree_for_poses_related_by_the_half_turn():
    cam = camera()
    v, f = rt.uv_sphere(12, 16, 1.0)
    v = v * np.array([1.0, 0.6, 0.8], dtype=np.float32)
    q = np.array([0.3, -0.5, 0.2, 0.7]); q /= np.linalg.norm(q)
    p = np.array([0.03, -0.05, -0.6])
    d_gl, f_gl, _ = rt.render_mesh((v, f), cam, (0.2, q, p), convention="opengl")
    # the same scene in the Open3D frame: the half turn about x, (1, 0, 0, 0) * q and (x, -y, -z)
    x, y, z, w = q
    q_o3d = np.array([w, -z, y, -x])     # (1,0,0,0) (x) q, scalar last
    d_o3d, f_o3d, _ = rt.render_mesh((v, f), cam, (0.2, q_o3d, p * [1, -1, -1]), convention="open3d")
    assert (d_gl > 0).sum() > 300
    assert np.array_equal(d_gl > 0, d_o3d > 0)
    assert np.max(np.abs(d_gl - d_o3d)) < 1e-13 and np.array_equal(f_gl, f_o3d)


def test_twin_lowest_index_wins_among_coincident_triangles_and_near():
    cam = camera()
    v = np.array([[-1, -1, 1.0], [1, -1, 1.0], [0, 1, 1.0], [-1, -1, 2.0], [1, -1, 2.0], [0, 1, 2.0]])
    f = np.array([[3, 4, 5], [0, 1, 2], [2, 1, 0], [0, 2, 1]])
    pose = (1.0, (0, 0, 0, 1), (0, 0, 0))
    depth, face, _ = rt.render_mesh((v, f), cam, pose, convention="open3d")
    assert set(np.unique(face)) == {-1, 1} and set(np.unique(depth)) == {0.0, 1.0}
    depth, face, _ = rt.render_mesh((v, f), cam, pose, convention="open3d", near=1.0)     # strict: depth > near
    assert set(np.unique(face)) == {-1, 0} and set(np.unique(depth)) == {0.0, 2.0}


@pytest.fixture(scope="module")
def L():
    from sdfest_amd import _lib
    _lib.build()
    return _lib.lib()


def test_mesh_depth_abi_argument_errors_without_gpu(L):
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)    # a non-NULL pointer that is never dereferenced
    err = lambda: L.sdfr_last_error()
    assert L.sdfr_mesh_depth_workspace_bytes(3, 100, 60, 640, 480) == 48     # 16 bytes per image
    assert L.sdfr_mesh_depth_workspace_bytes(0, 100, 60, 640, 480) == 0
    assert L.sdfr_mesh_depth_workspace_bytes(1, 0, 1, 640, 480) == 0
    assert L.sdfr_mesh_depth_workspace_bytes(1, 10, 11, 640, 480) == 0
    assert L.sdfr_mesh_depth_workspace_bytes(1, 10, 10, 0, 480) == 0

    def call(m=q, K=1, tf=10, mf=10, W=64, H=48, cx=32.0, cy=24.0, fx=60.0, fy=60.0, near=0.0, flags=0, d=q, t=None,
             ws=q, wb=1 << 20):
        return L.sdfr_mesh_depth(m, K, tf, mf, W, H, cx, cy, fx, fy, near, flags, d, t, ws, wb, 0, None)

    assert call(K=0) == -1 and b"K=0" in err()
    assert call(K=65536) == -1
    assert call(tf=0, mf=1) == -1 and b"total_faces" in err()
    assert call(mf=11) == -1 and b"max_faces" in err()
    assert call(W=0) == -1 and b"W=0" in err()
    assert call(H=-3) == -1
    assert call(fx=0.0) == -1 and b"fx" in err()
    assert call(fy=float("nan")) == -1
    assert call(cx=float("inf")) == -1 and b"cx" in err()
    assert call(near=-0.1) == -1 and b"near" in err()
    assert call(near=float("nan")) == -1
    assert call(flags=2) == -1 and b"flags" in err()
    for kw in ("m", "d", "ws"):
        assert call(**{kw: None}) == -2, kw
    assert call(K=2, tf=20, wb=31) == -3 and b"workspace" in err()


def test_render_mesh_depth_rejects_bad_arguments_before_the_gpu():
    from sdfest_amd import Camera, Mesh, draw_depth_geometry, render_mesh_depth
    m = Mesh(torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="skew"):
        draw_depth_geometry(m, Camera(64, 48, 60.0, 60.0, 32.0, 24.0, s=0.1, pixel_center=0.5))
    with pytest.raises(ValueError, match="convention"):
        render_mesh_depth(m, camera(), convention="vulkan")
    with pytest.raises(ValueError, match="near"):
        render_mesh_depth(m, camera(), near=-1.0)
    with pytest.raises(TypeError, match="CUDA"):
        render_mesh_depth(m, camera())
    with pytest.raises(ValueError, match="no meshes"):
        render_mesh_depth([], camera())


OBJ_TEXT = """# every corner form
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0 0
vn 0 0 1
v 0.5 0.5 1   # a comment after data
f 1 2 3
f 1/1 3/1 4/1
f 1/1/1 2/1/1 5/1/1
f 2//1 3//1 5//1
f -5 -4 -3 -2
g ignored
f -1 -2 -3
"""


def test_from_file_obj_index_forms_polygons_and_negative_indices(tmp_path):
    from sdfest_amd import Mesh
    path = tmp_path / "forms.obj"
    path.write_text(OBJ_TEXT)
    m = Mesh.from_file(str(path), scale=1, rel_scale=True, device="cpu")
    assert m.vertices.dtype == torch.float32 and m.faces.dtype == torch.int32 and m.normals is None
    assert np.array_equal(m.vertices.numpy(), np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]],
                                                       dtype=np.float32))
    assert m.faces.numpy().tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [0, 1, 2], [0, 2, 3], [4, 3, 2]]
    # scale: absolute = half the largest extent, relative = a factor
    assert Mesh.from_file(str(path), scale=0.25, rel_scale=False, device="cpu")._factor == pytest.approx(0.5)
    assert Mesh.from_file(str(path), scale=0.25, rel_scale=True, device="cpu")._factor == 0.25
    # center: the vertex mean goes to the origin
    c = Mesh.from_file(str(path), rel_scale=True, center=True, device="cpu")
    assert np.allclose(c.vertices.numpy().mean(0), 0, atol=1e-7)
    assert np.allclose(c.vertices.numpy(), m.vertices.numpy() - m.vertices.numpy().mean(0), atol=1e-7)
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError, match="vertex"):
        Mesh.from_file(str(bad), device="cpu")


@pytest.mark.parametrize("with_normals", [False, True])
def test_from_file_round_trips_write_obj_and_write_ply(tmp_path, with_normals):
    from sdfest_amd import Mesh
    v, f = rt.uv_sphere(7, 9, 0.3)
    n = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32) if with_normals else None
    m = Mesh(torch.from_numpy(v), torch.from_numpy(f), None if n is None else torch.from_numpy(n), scale=1.0,
             rel_scale=True)
    for ext, write in (("obj", m.write_obj), ("ply", m.write_ply)):
        path = str(tmp_path / f"mesh.{ext}")
        write(path)
        back = Mesh.from_file(path, scale=1, rel_scale=True, device="cpu")
        assert np.array_equal(back.vertices.numpy(), v), ext      # %.9g and raw float32 are both exact
        assert np.array_equal(back.faces.numpy(), f), ext
        if with_normals:
            assert np.array_equal(back.normals.numpy(), n), ext
        else:
            assert back.normals is None


def test_from_file_ascii_ply_with_a_quad(tmp_path):
    from sdfest_amd import Mesh
    path = tmp_path / "quad.ply"
    path.write_text("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 4\nproperty float x\nproperty float y\n"
                    "property float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
                    "0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    m = Mesh.from_file(str(path), rel_scale=True, device="cpu")
    assert m.faces.numpy().tolist() == [[0, 1, 2], [0, 2, 3]] and m.vertices.shape == (4, 3)


def test_view_poses_match_the_reference_algebra():
    """evaluation.view_poses against tests/golden/eval_views.npz (tools/make_view_goldens.py: the lines of the
    reference's _generate_views with the reference's own quaternion functions), on CPU tensors in float64"""
    from sdfest_amd.evaluation import view_poses
    g = np.load(os.path.join(GOLDEN, "eval_views.npz"))
    for i in range(len(g["camera_distances"])):
        dist = float(g["camera_distances"][i])
        cam_p, mesh_p, mesh_q = view_poses(torch.tensor(g["camera_orientations"][i:i + 1]),
                                           torch.tensor(g["mesh_orientations"][i]), dist)
        assert np.allclose(cam_p.numpy()[0], g["camera_positions"][i], atol=1e-12), i
        assert np.allclose(mesh_q.numpy()[0], g["mesh_orientations_cam"][i], atol=1e-12), i
        assert np.array_equal(mesh_p.numpy()[0], [0.0, 0.0, dist])
    # all cameras at once equal one by one
    cam_p, _, mesh_q = view_poses(torch.tensor(g["camera_orientations"][3:7]), torch.tensor(g["mesh_orientations"][3]), 0.5)
    one = view_poses(torch.tensor(g["camera_orientations"][5:6]), torch.tensor(g["mesh_orientations"][3]), 0.5)
    assert torch.equal(cam_p[2], one[0][0]) and torch.equal(mesh_q[2], one[2][0])


def test_view_poses_put_the_mesh_on_the_principal_axis():
    """independent of the golden: the world origin, seen from the camera, lies at (0, 0, -d) in its OpenGL frame, and a
    mesh point maps to the same place through the world and through the Open3D-frame pose"""
    from sdfest_amd.evaluation import view_poses
    from sdfest_amd.pipeline import quaternion_apply, quaternion_invert
    gen = torch.Generator().manual_seed(3)
    q = torch.randn((5, 4), generator=gen, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True)
    mq = torch.tensor([0.2, -0.4, 0.1, 0.8], dtype=torch.float64)
    mq = mq / mq.norm()
    cam_p, mesh_p, mesh_q = view_poses(q, mq, 0.7)
    origin_in_cam = quaternion_apply(quaternion_invert(q), -cam_p)
    assert torch.allclose(origin_in_cam, torch.tensor([0.0, 0.0, -0.7], dtype=torch.float64).expand(5, 3), atol=1e-12)
    x = torch.tensor([0.3, -0.2, 0.5], dtype=torch.float64).expand(5, 3)
    world = quaternion_apply(mq.expand(5, 4), x)
    in_gl = quaternion_apply(quaternion_invert(q), world - cam_p)
    in_o3d = quaternion_apply(mesh_q, x) + mesh_p
    assert torch.allclose(in_gl * torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64), in_o3d, atol=1e-12)


def test_metric_stats_are_the_population_statistics():
    from sdfest_amd.evaluation import metric_stats
    s = metric_stats([{"a": 1.0, "b": 2.0}, {"a": 3.0, "b": 2.0}, {"a": 5.0, "b": 2.0}])
    assert s["a"] == {"mean": 3.0, "var": pytest.approx(8.0 / 3), "std": pytest.approx((8.0 / 3) ** 0.5)}
    assert s["b"] == {"mean": 2.0, "var": 0.0, "std": 0.0}
