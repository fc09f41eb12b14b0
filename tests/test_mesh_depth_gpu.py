"""GPU: the mesh depth rasteriser (``sdfr_mesh_depth``, csrc/raster.hip, ``sdfest_amd.render_mesh_depth``) against its
float64 CPU twin tests/raster_twin.py.

Which of two neighbouring triangles covers a pixel cannot be held to the twin (float32 moves an edge by 1e-4 .. 1e-2 of
a triangle), but the image can: the twin's `bracket` renders the pixel-centre ray and four rays 1/32 pixel beside it, and
the kernel's depth must lie within [lo (1 - 1e-5), hi (1 + 1e-5)] of those five, be exactly 0 where all five miss and
> 0 where all five hit.  Two caps keep the bracket from hiding a failure: at most 1 % of a scene's pixels are `mixed`,
at least 5 % of its hit pixels are `flat` -- there the kernel's depth is held to 4 x the error the twin itself makes in
float32.  The scenes (tests/raster_scenes.py) were checked against both caps on the CPU before any GPU run.

Measured on the MI355X, maximum relative depth error on flat pixels, kernel / float32 twin: a_sphere_160 1.96e-7 /
1.59e-7, a_blobs_160_open3d 2.82e-7 / 1.92e-7, a_blobs_640 3.02e-7 / 4.99e-7, b_cube_fills_image 1.69e-7 / 2.19e-7,
b_camera_inside_cube 1.59e-7 / 2.15e-7, c_partly_behind_offscreen 3.44e-7 / 3.84e-7, d_fine_sphere_204k 2.19e-7 /
1.55e-7, e_ragged_offcentre 1.36e-7 / 1.03e-7, f_near_cuts_the_sphere 2.54e-7 / 1.90e-7; no bracket violation in any
scene.  Mesh against sphere tracer: median |difference| 2.26e-4 m, maximum 7.13e-4 m, bound 2.28e-2 m (DESIGN.md
section 3.12)."""
import numpy as np
import pytest
import torch

import raster_scenes as rs
import raster_twin as rt

pytestmark = pytest.mark.gpu

T = lambda a, dt=torch.float32: torch.tensor(np.asarray(a), dtype=dt, device="cuda")
_MC = {}


def mc(name):
    """the marching-cubes mesh of sphere_sdf / blobs_sdf at level 0, from the GPU, as numpy"""
    if name not in _MC:
        from sdfest_amd import extract_mesh
        from sdfest_amd.synthetic import blobs_sdf, sphere_sdf
        sdf = {"sphere": sphere_sdf(0.5, 64), "blobs": blobs_sdf(0)}[name]
        m = extract_mesh(torch.tensor(sdf, device="cuda"), 0.0)
        _MC[name] = (m.vertices.cpu().numpy(), m.faces.cpu().numpy())
    return _MC[name]


def gpu_mesh(mesh, factor=1.0, quat=(0, 0, 0, 1), position=(0, 0, 0)):
    from sdfest_amd import Mesh
    v, f = mesh
    return Mesh(T(v), T(f, torch.int32), scale=factor, rel_scale=True, position=T(position), orientation=T(quat))


def gpu_render(scene, **kw):
    from sdfest_amd import render_mesh_depth
    m = gpu_mesh(scene["mesh"], *scene["pose"])
    return render_mesh_depth(m, scene["camera"], convention=scene["convention"], near=scene["near"], **kw)


SCENES = None


def all_scenes():
    global SCENES
    if SCENES is None:
        SCENES = {s["name"]: s for s in rs.scenes(mc)}
    return SCENES


SCENE_NAMES = ["a_sphere_160", "a_blobs_160_open3d", "a_blobs_640", "b_cube_fills_image", "b_camera_inside_cube",
               "c_partly_behind_offscreen", "c_wholly_behind", "d_fine_sphere_204k", "e_ragged_offcentre",
               "f_near_cuts_the_sphere"]


def test_scene_list_is_complete():
    assert sorted(all_scenes()) == sorted(SCENE_NAMES)
    assert len(all_scenes()["d_fine_sphere_204k"]["mesh"][1]) >= 200_000


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_kernel_within_the_twin_bracket(name):
    s = all_scenes()[name]
    depth, tri = gpu_render(s, return_triangles=True)
    torch.cuda.synchronize()
    assert depth.dtype == torch.float32 and tri.dtype == torch.int32
    W, H = s["camera"].width, s["camera"].height
    assert tuple(depth.shape) == (1, H, W) == tuple(tri.shape)
    g, gt = depth[0].cpu().numpy().astype(np.float64), tri[0].cpu().numpy()
    b = rt.bracket(s["mesh"], s["camera"], s["pose"], convention=s["convention"], near=s["near"])
    hit = b["depth"] > 0
    n_hit = int(hit.sum())
    # the caps (conditions on the scene, evaluated with the twin alone)
    mixed_share = b["mixed"].mean()
    flat_share = b["flat"].sum() / max(n_hit, 1)
    print(f"{name}: F={len(s['mesh'][1])} hit={n_hit} mixed={100 * mixed_share:.3f}% flat/hit={100 * flat_share:.1f}%")
    assert mixed_share <= 0.01
    if s["flat"]:
        assert n_hit > 200 and flat_share >= 0.05
    if name == "c_wholly_behind":
        assert n_hit == 0 and not g.any() and (gt == -1).all()
        return
    # depth and hit / miss, every pixel
    assert np.isfinite(g).all() and (g >= 0).all()
    assert ((gt >= 0) == (g > 0)).all() and gt.max() < len(s["mesh"][1])
    low, high = b["lo"] * (1 - 1e-5), b["hi"] * (1 + 1e-5)
    bad = (g < low) | (g > high)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5], g[bad][:5], b["lo"][bad][:5], b["hi"][bad][:5])
    assert not g[b["none"]].any() and (g[b["all"]] > 0).all()
    if s["near"] > 0:
        assert g[g > 0].min() > s["near"]
    # depth values on flat pixels: 4 x what the twin itself loses in float32
    fl = b["flat"]
    d32 = rt.render_mesh(s["mesh"], s["camera"], s["pose"], s["convention"], s["near"], dtype=np.float32)[0]
    ref = b["depth"][fl]
    twin32 = np.max(np.abs(d32[fl].astype(np.float64) / ref - 1))
    kernel = np.max(np.abs(g[fl] / ref - 1))
    both = hit & (g > 0)
    print(f"{name}: flat pixels {int(fl.sum())}: kernel {kernel:.2e}, float32 twin {twin32:.2e}; all hit pixels: kernel "
          f"{np.max(np.abs(g[both] / b['depth'][both] - 1)):.2e}")
    assert twin32 > 0
    assert kernel <= 4 * twin32, (kernel, twin32)
    # the face index where it is well defined
    if s["faces"]:
        ok = b["face_ok"]
        print(f"{name}: face index well defined on {int(ok.sum())} of {n_hit} hit pixels")
        if s["kind"] in "ab":
            assert ok.sum() >= n_hit / 3
        assert ok.any() and np.array_equal(gt[ok], b["face"][ok])


def test_lowest_index_wins_among_coincident_triangles():
    from sdfest_amd import Camera
    cam = Camera(64, 48, 60.0, 60.0, 32.0, 24.0, pixel_center=0.5)
    v = np.array([[-1, -1, -1.0], [1, -1, -1.0], [0, 1, -1.0], [-1, -1, -2.0], [1, -1, -2.0], [0, 1, -2.0]], np.float32)
    f = np.array([[3, 4, 5], [0, 1, 2], [2, 1, 0], [0, 2, 1]], np.int32)
    depth, tri = gpu_mesh((v, f)).render_depth(cam, return_triangles=True)
    d, t = depth.cpu().numpy(), tri.cpu().numpy()
    assert depth.shape == (48, 64)
    assert set(np.unique(t)) == {-1, 1} and set(np.unique(d)) == {0.0, 1.0}
    depth, tri = gpu_mesh((v, f)).render_depth(cam, near=1.0, return_triangles=True)     # strict: depth > near
    assert set(np.unique(tri.cpu().numpy())) == {-1, 0} and set(np.unique(depth.cpu().numpy())) == {0.0, 2.0}
    tw = rt.render_mesh((v, f), cam, (1.0, (0, 0, 0, 1), (0, 0, 0)))
    assert np.array_equal(t, tw[1])


def test_shared_edges_leave_no_cracks():
    """a closed fine sphere seen from outside: every pixel strictly inside the silhouette is hit (a pixel centre on a
    shared edge is covered by one of the two triangles), whatever the triangle order"""
    s = all_scenes()["d_fine_sphere_204k"]
    g = gpu_render(s)[0].cpu().numpy()
    W, H, fx, fy, cx, cy = rt.camera_params(s["camera"])
    col, row = np.meshgrid(np.arange(W), np.arange(H))
    d = np.stack([(col + 0.5 - cx) / fx, -(row + 0.5 - cy) / fy, -np.ones((H, W))], -1)
    c = np.array(s["pose"][2])
    r = s["pose"][0] * 0.9998       # inside the tessellation's inscribed sphere (cos(pi / 320) cos(pi / 640) = 0.99994)
    t = d @ c
    inside = t * t - (d * d).sum(-1) * (c @ c - r * r) > 0
    assert inside.sum() > 5000 and (g[inside] > 0).all()


def test_bad_triangles_leave_the_valid_image_bitwise_unchanged():
    """degenerate, NaN and out-of-range-index triangles mixed into a valid mesh"""
    from sdfest_amd import render_mesh_depth
    s = all_scenes()["a_sphere_160"]
    v, f = s["mesh"]
    nv = len(v)
    extra_v = np.array([[np.nan, 0, 0], [np.inf, 0.1, 0.2], [0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [0.0, 0.0, 0.0],
                        [0.1, 0.1, 0.1], [0.2, 0.2, 0.2]], np.float32)
    v2 = np.concatenate([v, extra_v])
    junk = np.array([[0, 1, nv], [2, nv + 1, 3],                       # a NaN and an infinite vertex
                     [0, 0, 1], [5, 6, 5], [7, 7, 7],                  # repeated indices
                     [nv + 2, nv + 3, 10], [nv + 3, 11, nv + 2],       # two vertices in one place
                     [nv + 4, nv + 5, nv + 6],                         # three on a line
                     [-1, 0, 1], [0, nv + 7, 1], [2, 3, 2 ** 31 - 1], [-2 ** 31, 4, 5],     # outside [0, V)
                     [nv + 100000, 1, 2]], np.int32)
    rng = np.random.default_rng(0)
    f2 = np.concatenate([f, junk])
    where = rng.permutation(len(f2))
    f2 = f2[where]
    clean = gpu_render(s)
    m2 = gpu_mesh((v2, f2), *s["pose"])
    dirty, tri = render_mesh_depth(m2, s["camera"], convention=s["convention"], return_triangles=True)
    assert torch.equal(clean, dirty)
    t = tri.cpu().numpy()
    valid = np.argsort(where)[:len(f)]      # positions of the valid faces in f2
    assert np.isin(t[t >= 0], valid).all()


def test_bitwise_reproducible_runs_permutations_and_batches():
    from sdfest_amd import render_mesh_depth
    s = all_scenes()["a_blobs_160_open3d"]
    v, f = s["mesh"]
    cam = s["camera"]
    first, tri = gpu_render(s, return_triangles=True)
    for _ in range(3):
        again, tri2 = gpu_render(s, return_triangles=True)
        assert torch.equal(first, again) and torch.equal(tri, tri2)
    # a permutation of the face list: the same depth bits, the same triangles under the permutation
    perm = np.random.default_rng(1).permutation(len(f))
    m = gpu_mesh((v, f[perm]), *s["pose"])
    dp, tp = render_mesh_depth(m, cam, convention=s["convention"], return_triangles=True)
    assert torch.equal(first, dp)
    # V poses of one mesh in one call = V single calls
    rng = np.random.default_rng(2)
    V = 7
    quats = np.stack([rs.random_quat(rng) for _ in range(V)]).astype(np.float32)
    pos = (np.array(s["pose"][2]) + rng.uniform(-0.02, 0.02, (V, 3))).astype(np.float32)
    base = gpu_mesh((v, f), s["pose"][0])
    batch, btri = render_mesh_depth(base, cam, T(pos), T(quats), convention="open3d", return_triangles=True)
    assert tuple(batch.shape) == (V, cam.height, cam.width)
    for k in range(V):
        one, otri = base.render_depth(cam, pos[k], quats[k], convention="open3d", return_triangles=True)
        assert one.shape == (cam.height, cam.width)
        assert torch.equal(batch[k], one) and torch.equal(btri[k], otri), k
        assert (one > 0).sum() > 1000
    # the mesh's own pose is what positions / orientations replace
    own = gpu_mesh((v, f), s["pose"][0], quats[3], pos[3])
    assert torch.equal(render_mesh_depth(own, cam, convention="open3d")[0], batch[3])


def test_different_meshes_in_one_call_and_out_buffer():
    from sdfest_amd import Mesh, draw_depth_geometry, render_mesh_depth
    sc = all_scenes()
    cam = sc["a_sphere_160"]["camera"]
    names = ["a_sphere_160", "b_cube_fills_image", "d_fine_sphere_204k", "f_near_cuts_the_sphere"]
    meshes = [gpu_mesh(sc[n]["mesh"], *sc[n]["pose"]) for n in names]
    empty = Mesh(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    meshes.insert(2, empty)
    out = torch.full((5, cam.height, cam.width), 7.0, device="cuda")
    res = render_mesh_depth(meshes, cam, out=out)
    assert res.data_ptr() == out.data_ptr()
    for k, m in enumerate(meshes):
        single = render_mesh_depth(m, cam)
        assert torch.equal(out[k], single[0]), k
    assert not out[2].any() and (out[0] > 0).sum() > 1000
    assert not render_mesh_depth(empty, cam).any()
    with pytest.raises(ValueError, match="out must be"):
        render_mesh_depth(meshes, cam, out=out[:4])
    # draw_depth_geometry: the reference's name and frame = the OpenGL image of the half-turned pose
    s = sc["a_blobs_160_open3d"]
    m = gpu_mesh(s["mesh"], *s["pose"])
    img = draw_depth_geometry(m, s["camera"])
    assert img.shape == (120, 160) and img.dtype == torch.float32 and img.is_cuda
    assert torch.equal(img, render_mesh_depth(m, s["camera"], convention="open3d")[0])
    x, y, z, w = s["pose"][1]
    gl = gpu_mesh(s["mesh"], s["pose"][0], (w, -z, y, -x), np.array(s["pose"][2]) * [1, -1, -1])
    img_gl = gl.render_depth(s["camera"])
    assert ((img > 0) != (img_gl > 0)).float().mean().item() < 2e-3
    both = (img > 0) & (img_gl > 0)
    assert (img[both] / img_gl[both] - 1).abs().median().item() < 1e-6


def test_replay_inside_a_captured_graph():
    from sdfest_amd import _lib, mesh as mesh_mod, render_mesh_depth
    s = all_scenes()["a_sphere_160"]
    cam = s["camera"]
    W, H, fx, fy, cx, cy = rt.camera_params(cam)
    m = gpu_mesh(s["mesh"], s["pose"][0], position=(0, 0, -0.5))
    K, F = 2, len(s["mesh"][1])
    tab = mesh_mod._MeshTable([m] * K, "render")
    tab.set_poses()
    table = tab.table
    assert (tab.total_faces, tab.max_faces) == (K * F, F)
    ws = torch.empty(_lib.lib().sdfr_mesh_depth_workspace_bytes(K, K * F, F, W, H), dtype=torch.uint8, device="cuda")
    depth = torch.zeros((K, H, W), device="cuda")
    launch = lambda: mesh_mod._mesh_depth_launch(table, K * F, F, (cx, cy, fx, fy), 0.0, 0, depth, None, ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                 # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    # new poses written in place, one replay
    quats = T([s["pose"][1], (0.0, 0.0, 0.0, 1.0)])
    pos = T([s["pose"][2], (0.01, 0.0, -0.45)])
    tab.quat[:], tab.position[:] = quats, pos
    depth.fill_(3.0)
    graph.replay()
    torch.cuda.synchronize()
    eager = render_mesh_depth(gpu_mesh(s["mesh"], s["pose"][0]), cam, pos, quats)
    assert torch.equal(depth, eager) and (depth[1] > 0).sum() > 1000


def test_mesh_image_against_the_sphere_tracer():
    """The cross-check that motivates the feature: sphere_sdf -> extract_mesh(level 0) -> render_mesh_depth against
    render_depth_gpu of the same grid at the same pose.  The marching-cubes surface and the trilinear zero set lie in
    the same grid cells, less than a cell diagonal c = 2 sqrt(3) scale / (R - 1) apart along the normal, i.e. at most
    c / k along a ray that meets the surface at angle cosine k, and the tracer stops up to threshold * depth / k early:
    on pixels hit in both images whose mesh triangle has k >= 0.5 none may differ by more than 2 (c + threshold *
    depth)."""
    from sdfest_amd import Camera, extract_mesh, render_depth_gpu
    from sdfest_amd.synthetic import sphere_sdf
    R, scale, thr = 64, 0.2, 0.001
    cam = Camera(160, 120, 150.0, 150.0, 80.0, 60.0, pixel_center=0.5)
    sdf = torch.tensor(sphere_sdf(0.5, R), device="cuda")
    q = T(rs.unit([0.2, -0.3, 0.1, 0.9]))
    p = T([0.03, -0.02, -0.4])
    m = extract_mesh(sdf, 0.0)
    m.update_scale(scale, rel_scale=True)
    m.position, m.orientation = p, q
    dm, tri = m.render_depth(cam, return_triangles=True)
    with torch.no_grad():
        dt = render_depth_gpu(sdf, p, q, torch.tensor(1.0 / scale, device="cuda"), None, None, None, thr, cam)
    dm, dt, tri = dm.cpu().numpy().astype(np.float64), dt.cpu().numpy().astype(np.float64), tri.cpu().numpy()
    both = (dm > 0) & (dt > 0)
    assert both.sum() > 1500 and ((dm > 0) != (dt > 0)).mean() < 0.03
    # the angle cosine between the pixel's ray and its mesh triangle's normal
    P = rt.pose_vertices(m.vertices.cpu().numpy(), scale, q.cpu().numpy(), p.cpu().numpy(), "opengl")
    f = m.faces.cpu().numpy()
    n = np.cross(P[f[:, 1]] - P[f[:, 0]], P[f[:, 2]] - P[f[:, 0]])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    W, H, fx, fy, cx, cy = rt.camera_params(cam)
    col, row = np.meshgrid(np.arange(W), np.arange(H))
    d = np.stack([(col + 0.5 - cx) / fx, (row + 0.5 - cy) / fy, np.ones((H, W))], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    k = np.abs((n[np.maximum(tri, 0)] * d).sum(-1))
    sel = both & (k >= 0.5)
    assert sel.sum() >= 0.5 * (dm > 0).sum()
    c = 2 * np.sqrt(3) * scale / (R - 1)
    diff = np.abs(dm - dt)[sel]
    print(f"mesh vs tracer: {int(sel.sum())} pixels, median |diff| {np.median(diff):.3e}, max {diff.max():.3e}, "
          f"cell diagonal {c:.3e}, bound at 0.4 m {2 * (c + thr * 0.4):.3e}")
    assert (diff <= 2 * (c + thr * dm[sel])).all()
