"""GPU: sdfr_render_normals / sdfr_depth_range / sdfr_shade_frames against closed forms and the float64 numpy twin
(tests/shading_twin.py).  Every shape here takes well under a second."""
import numpy as np
import pytest
import torch

import shading_twin as T
from helpers import load_render_case
from test_shading_cpu import PLANE_A, PLANE_Q, plane_sdf

pytestmark = pytest.mark.gpu

WHITE = [255, 255, 255]


def dev(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


@pytest.fixture(scope="module")
def V():
    assert torch.cuda.is_available()
    import sdfest_amd.visualization as v
    return v


@pytest.fixture(scope="module")
def table():
    return T.load_table()


def camera_of(c):
    from sdfest_amd import Camera
    return Camera(c["W"], c["H"], c["fx"], c["fy"], c["cx"], c["cy"], pixel_center=0.5)


def pose_of(c):
    return (dev(np.reshape(c["p"], (1, 3))), dev(np.reshape(c["q"], (1, 4))), dev(np.reshape(c["inv_scale"], (1,))))


_scene_cache = {}


def scene(V, name):
    """(case, camera, sdf, pose tensors, GPU depth (H,W) numpy float32, GPU normals (H,W,3) numpy): rendered once per
    scene and shared, unchanged, by the tests that need it"""
    if name not in _scene_cache:
        from sdfest_amd import render_depth_batch
        c = load_render_case(name)
        cam = camera_of(c)
        sdf = dev(c["sdf"])
        pos, quat, isc = pose_of(c)
        depth = render_depth_batch(sdf, pos, quat, isc, c["thr"], cam)
        normals = V.render_normals(sdf, pos, quat, isc, c["thr"], cam, depth=depth)
        _scene_cache[name] = (c, cam, sdf, (pos, quat, isc), depth, depth[0].cpu().numpy(), normals[0].cpu().numpy())
    return _scene_cache[name]


def twin_of(c, depth):
    return T.normals(depth, c["sdf"], c["p"], c["q"], c["inv_scale"], c["cx"], c["cy"], c["fx"], c["fy"])


def test_plane_normal_is_the_rotated_plane_normal(V):
    """a . x - c on an R = 8 grid: the interpolant is the field, its gradient the same in every cell, so EVERY hit pixel
    has the normal R(q) a / |a| -- no exclusions.  Catches a transposed rotation, a sign error and an axis permutation,
    which a twin sharing the mistake would not."""
    from sdfest_amd import Camera, render_depth_batch
    cam = Camera(33, 25, 30.0, 29.0, 16.5, 12.5, pixel_center=0.5)
    sdf = dev(plane_sdf())
    pos, quat, isc = dev([[0.05, -0.1, -1.6]]), dev(PLANE_Q[None]), dev([1.3])
    depth = render_depth_batch(sdf, pos, quat, isc, 0.005, cam)
    n = V.render_normals(sdf, pos, quat, isc, 0.005, cam, depth=depth)[0].cpu().numpy()
    hit = depth[0].cpu().numpy() != 0
    assert hit.sum() > 100 and (~hit).sum() > 20
    expect = T.rotation(PLANE_Q) @ (PLANE_A / np.linalg.norm(PLANE_A))
    err = np.max(np.abs(n[hit] - expect))
    print("plane: hit pixels", int(hit.sum()), "max |n - R a/|a||", err)
    assert err <= 1e-5
    assert not n[~hit].any()
    # depth=None renders the same depth itself
    n2 = V.render_normals(sdf, pos, quat, isc, 0.005, cam)[0].cpu().numpy()
    assert np.array_equal(n, n2)


def test_sphere_normals_point_away_from_the_centre(V):
    c, cam, sdf, pose, _, depth, n = scene(V, "g1_sphere_64x48")
    _, info = twin_of(c, depth)
    hit = depth != 0
    assert hit.sum() > 200
    radial = info["point"] @ T.rotation(c["q"]).T          # centre -> hit point, camera frame
    radial = radial / np.linalg.norm(radial, axis=-1, keepdims=True)
    cos = np.sum(n * radial, -1)[hit]
    print("sphere: min cosine", cos.min())
    assert cos.min() > 0.99
    assert np.max(np.abs(np.linalg.norm(n[hit], axis=-1) - 1)) < 1e-5


@pytest.mark.parametrize("name", T.TWIN_SCENES)
def test_normals_match_the_twin(V, name):
    c, cam, sdf, pose, _, depth, n = scene(V, name)
    n64, info = twin_of(c, depth)
    hit = depth != 0
    assert hit.sum() > 50, name
    left_out = T.excluded(info)
    share = left_out.sum() / hit.sum()
    keep = hit & ~left_out
    bound = max(1e-4, 10 * T.load_floors()[name])
    worst = float(np.max(T.angles(n, n64)[keep]))
    print(f"{name}: hit {int(hit.sum())}, left out {100 * share:.2f} %, worst angle {worst:.3e} rad, bound {bound:.1e}")
    assert share <= 0.05
    assert worst <= bound
    assert not n[~hit].any()
    # the pixels left out still hold unit normals (or zeros), never garbage
    lengths = np.linalg.norm(n[hit], axis=-1)
    assert np.all((np.abs(lengths - 1) < 1e-5) | (lengths == 0))


@pytest.mark.parametrize("name", ["g4_behind_32x24", "g4_offscreen_32x24"])
def test_empty_scenes(V, name):
    c, cam, sdf, (pos, quat, isc), depth_t, depth, n = scene(V, name)
    assert not depth.any()
    assert not n.any()
    frames = V.shade_frames(depth_t, sdf, pos, quat, isc, cam, target=depth_t)
    assert sorted(frames) == ["depth", "depth_error", "shaded"]
    for img in frames.values():
        img = img.cpu().numpy()
        assert img.shape == (1, c["H"], c["W"], 3) and img.dtype == np.uint8
        assert (img == 255).all()
    assert V.depth_range(depth_t).cpu().numpy().tolist() == [[0.0, 0.0]]


def test_batch_and_repeat(V):
    """six frames = three states with a grid each x two views: frame f is bitwise the single-frame call with its own
    grid, pose and target; a second call gives the same bits; five frames with two views per state are refused"""
    from sdfest_amd import Camera, render_depth_batch
    from sdfest_amd.synthetic import blobs_sdf
    cam = Camera(66, 50, 60.0, 60.0, 33.0, 25.0, pixel_center=0.5)     # 3300 pixels: a multiple of 4, rows are not
    grids = dev(np.stack([blobs_sdf(s) for s in (0, 1, 2)]))
    view_pos = np.array([[0.0, 0.05, -1.5], [0.1, -0.05, -1.7]])
    view_quat = np.array([[0.0, 0.0, 0.0, 1.0], [0.18, -0.31, 0.45, 0.82]])
    view_quat /= np.linalg.norm(view_quat, axis=1, keepdims=True)
    pos, quat = dev(np.tile(view_pos, (3, 1))), dev(np.tile(view_quat, (3, 1)))
    isc = dev([2.0, 2.1, 1.9, 2.0, 2.2, 2.05])
    per_frame = grids.repeat_interleave(2, 0).contiguous()
    depth = render_depth_batch(per_frame, pos, quat, isc, 0.005, cam)
    target = (depth[:2] * 1.01).contiguous()
    target[0, :10] = 0
    rng = dev([[1.0, 2.2]])
    with pytest.raises(RuntimeError):
        V.shade_frames(depth[:5].contiguous(), grids, pos[:5].contiguous(), quat[:5].contiguous(),
                       isc[:5].contiguous(), cam, target=target, views_per_state=2, value_range=rng)
    with pytest.raises(RuntimeError):
        V.shade_frames(depth[:5].contiguous(), None, None, None, None, cam, target=target, views_per_state=2,
                       value_range=rng, outputs=("depth", "depth_error"))
    call = lambda: V.shade_frames(depth, grids, pos, quat, isc, cam, target=target, views_per_state=2, value_range=rng)
    first, second = call(), call()
    normals = V.render_normals(per_frame, pos, quat, isc, 0.005, cam, depth=depth)
    assert (depth != 0).sum(dim=(1, 2)).min().item() > 100
    for f in range(6):
        s = slice(f, f + 1)
        alone = V.shade_frames(depth[s], grids[f // 2], pos[s], quat[s], isc[s], cam, target=target[f % 2:f % 2 + 1],
                               views_per_state=1, value_range=rng)
        for name in T_OUTPUTS:
            assert torch.equal(first[name][f], alone[name][0]), (name, f)
            assert torch.equal(first[name], second[name]), name
        n1 = V.render_normals(grids[f // 2], pos[s], quat[s], isc[s], 0.005, cam, depth=depth[s])
        assert torch.equal(normals[f], n1[0]), f
    # per-frame ranges: frame f with row f
    rows = V.depth_range(depth)
    per = V.shade_frames(depth, None, None, None, None, cam, value_range=rows, outputs=("depth",))["depth"]
    for f in (0, 5):
        one = V.shade_frames(depth[f:f + 1], None, None, None, None, cam, value_range=rows[f], outputs=("depth",))
        assert torch.equal(per[f], one["depth"][0])


T_OUTPUTS = ("depth", "depth_error", "shaded")


@pytest.mark.parametrize("shape", [(1, 1), (25, 33), (120, 160)])
def test_depth_range_equals_numpy(V, shape):
    H, W = shape
    rng = np.random.default_rng(H * W)
    imgs = rng.uniform(0.3, 4.0, (5, H, W)).astype(np.float32)
    imgs[0] = 0.0                                     # no valid pixel: (0, 0)
    imgs[1][rng.random((H, W)) < 0.5] = 0.0
    flat = imgs[2].reshape(-1)
    flat[::3] = np.inf
    flat[1::5] = np.nan
    flat[2::7] = -np.inf
    imgs[3] *= -1.0                                   # negative values are values
    imgs[4][rng.random((H, W)) < 0.9] = 0.0
    d = dev(imgs)
    rows = V.depth_range(d).cpu().numpy()
    assert rows.shape == (5, 2) and rows.dtype == np.float32
    for b in range(5):
        assert tuple(rows[b].tolist()) == T.value_range(imgs[b]), b
    assert rows[0].tolist() == [0.0, 0.0]
    shared = V.depth_range(d, shared=True).cpu().numpy()
    assert shared.shape == (1, 2) and tuple(shared[0].tolist()) == T.value_range(imgs)
    assert tuple(V.depth_range(d[:1], shared=True).cpu().numpy()[0].tolist()) == (0.0, 0.0)
    assert tuple(V.depth_range(d[2], shared=True).cpu().numpy()[0].tolist()) == T.value_range(imgs[2])
    # the library's own shared form (one workgroup over all images) agrees with the two-launch form
    from sdfest_amd import _lib
    out = torch.empty((1, 2), device="cuda")
    _lib.check(_lib.lib().sdfr_depth_range(d.data_ptr(), 5, W, H, 1, out.data_ptr(), 0,
                                           torch.cuda.current_stream().cuda_stream), "sdfr_depth_range")
    assert np.array_equal(out.cpu().numpy(), shared)


def test_colour_lookup_rules(V, table):
    from sdfest_amd import Camera
    cam = Camera(16, 16, 16.0, 16.0, 8.0, 8.0, pixel_center=0.5)
    vmin, vmax = 1.0, 3.0                              # (i + 0.5) / 128 is exact in float32: no bin is in doubt
    centres = (vmin + (np.arange(256) + 0.5) / 256 * (vmax - vmin)).astype(np.float32).reshape(1, 16, 16)
    shade = lambda d, **kw: {k: v.cpu().numpy() for k, v in
                             V.shade_frames(dev(d), None, None, None, None, cam, **kw).items()}
    out = shade(centres, value_range=dev([vmin, vmax]), outputs=("depth",))["depth"]
    assert np.array_equal(out.reshape(256, 3), table)
    # the range as two numbers, as a (1,2) tensor and as one row per frame is the same range; other shapes are refused
    for form in ((vmin, vmax), dev([[vmin, vmax]]), torch.tensor([vmin, vmax])):
        assert np.array_equal(shade(centres, value_range=form, outputs=("depth",))["depth"], out)
    with pytest.raises(RuntimeError, match="value_range"):
        shade(centres, value_range=dev([vmin, vmax, 4.0]), outputs=("depth",))
    with pytest.raises(RuntimeError, match="value_range"):
        shade(centres, value_range=dev([[vmin, vmax], [vmin, vmax]]), outputs=("depth",))
    # vmax == vmin: entry 0 everywhere
    out = shade(centres, value_range=dev([2.0, 2.0]), outputs=("depth",))["depth"]
    assert np.array_equal(out.reshape(256, 3), np.broadcast_to(table[0], (256, 3)))
    # values outside the range clamp; zero depth is the background, whatever the background is
    d = centres.copy()
    d[0, 0, :4] = [0.5, 5.0, 0.0, -2.0]
    out = shade(d, value_range=dev([vmin, vmax]), outputs=("depth",), background=(1, 2, 3))["depth"][0]
    assert np.array_equal(out[0, 0], table[0]) and np.array_equal(out[0, 1], table[255])
    assert out[0, 2].tolist() == [1, 2, 3] and np.array_equal(out[0, 3], table[0])
    # the error image: bins of |d - t| / error_max at their centres, background where the target or the depth is 0
    e_max = 0.5
    err = ((np.arange(256) + 0.5) / 256 * e_max).reshape(1, 16, 16)
    t = (centres.astype(np.float64) + err * np.where(np.arange(256).reshape(1, 16, 16) % 2, 1, -1)).astype(np.float32)
    sure = np.abs(np.abs(centres.astype(np.float64) - t) / e_max * 256 - (np.arange(256).reshape(1, 16, 16) + 0.5)) < 0.25
    assert sure.all()
    t[0, 1, :3] = 0.0
    d = centres.copy()
    d[0, 2, :3] = 0.0
    out = shade(d, target=dev(t), error_max=e_max, outputs=("depth_error",))["depth_error"][0]
    expect = table.reshape(16, 16, 3).copy()
    expect[1, :3] = WHITE
    expect[2, :3] = WHITE
    assert np.array_equal(out, expect)
    # value_range=None: the shared range of the target where there is one, else of the depth
    auto = shade(d, target=dev(t), outputs=("depth",))["depth"]
    lo, hi = T.value_range(t)
    assert np.array_equal(auto, shade(d, value_range=dev([lo, hi]), outputs=("depth",))["depth"])
    auto = shade(d, outputs=("depth",))["depth"]
    lo, hi = T.value_range(d)
    assert np.array_equal(auto, shade(d, value_range=dev([lo, hi]), outputs=("depth",))["depth"])


@pytest.mark.parametrize("shape", [(25, 33), (120, 160)])
def test_random_depths_against_the_twin(V, table, shape):
    """a bin edge may fall either way in float32: every channel within the table's largest step between neighbours"""
    from sdfest_amd import Camera
    H, W = shape
    cam = Camera(W, H, 50.0, 50.0, W / 2, H / 2, pixel_center=0.5)
    rng = np.random.default_rng(7)
    d = rng.uniform(0.4, 3.0, (3, H, W)).astype(np.float32)
    d[rng.random(d.shape) < 0.3] = 0.0
    t = rng.uniform(0.4, 3.0, (1, H, W)).astype(np.float32)
    t[rng.random(t.shape) < 0.2] = 0.0
    t = np.where(rng.random(t.shape) < 0.5, d[:1] * 1.01, t).astype(np.float32)
    out = V.shade_frames(dev(d), None, None, None, None, cam, target=dev(t), value_range=dev([0.6, 2.7]),
                         error_max=0.05, outputs=("depth", "depth_error"))
    step = T.table_step(table)
    for f in range(3):
        got = out["depth"][f].cpu().numpy().astype(int)
        ref = T.depth_bytes(d[f], np.float32(0.6), np.float32(2.7), table).astype(int)
        assert np.max(np.abs(got - ref)) <= step
        assert np.mean(np.any(got != ref, -1)) < 0.01          # ... and almost all of them are equal
        assert np.array_equal(np.all(got == 255, -1), d[f] == 0)
        got = out["depth_error"][f].cpu().numpy().astype(int)
        ref = T.error_bytes(d[f], t[0], np.float32(0.05), table).astype(int)
        assert np.max(np.abs(got - ref)) <= step
        assert np.array_equal(np.all(got == 255, -1), (d[f] == 0) | (t[0] == 0))


@pytest.mark.parametrize("name", ["g3_pose1_64x48", "g4_parallel_slab_33x25", "g2_blobs_c1_160x120"])
def test_shaded_bytes_against_the_twin(V, name):
    c, cam, sdf, (pos, quat, isc), depth_t, depth, n = scene(V, name)
    light = (0.3, 0.5, 0.8)
    out = V.shade_frames(depth_t, sdf, pos, quat, isc, cam, light=light, outputs=("shaded",))["shaded"][0].cpu().numpy()
    n64, info = twin_of(c, depth)
    hit = depth != 0
    keep = hit & ~T.excluded(info)
    ref = T.shade_bytes(n64, light=light)
    diff = np.abs(out.astype(int) - ref.astype(int))
    print(name, "max byte difference", diff[keep].max())
    assert diff[keep].max() <= 1
    # the hit / background pattern is depth != 0 exactly (no shade reaches white: the base colour's largest is 0.7)
    assert np.array_equal(np.all(out == 255, -1), ~hit)
    # the shaded image is the shade of the normal map's own normals
    own = T.shade_bytes(n, light=light)
    assert np.abs(out.astype(int) - own.astype(int))[hit].max() <= 1
