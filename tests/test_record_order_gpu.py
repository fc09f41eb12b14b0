"""GPU: the face-record order of the packed march (device.hpp, record_index).

A grid shared by >= 17 views (SDFR_PACKED_MIN_VIEWS) is marched through its packed face records, fewer views through
the plain grid.  Both forms do the same arithmetic on the same corner values, so the depth of 17 views rendered in one
call equals, bit for bit, the depth of the same views rendered in calls of at most 16 -- whatever the order of the
records, for every way the index is formed: the bit path of R = 64, the integer path of other powers of two, of even and
of odd R.  (tests/test_render_gpu.py::test_packed_record_path_generic_and_odd_resolution holds the two forms to the same
bitwise equality at R = 33, 48 and 7 since before the 2 x 2 x 2 order.)"""
import numpy as np
import pytest
import torch

import oracle
from helpers import rel_err

pytestmark = pytest.mark.gpu

REL = 1e-4   # tests/test_render_gpu.py
VIEWS = 17
SIZES = ((32, 24), (48, 32))
RESOLUTIONS = (8, 9, 12, 16, 33, 64)


@pytest.fixture(scope="module")
def R():
    import sdfest_amd.differentiable_renderer as r
    assert torch.cuda.is_available()
    return r


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def unit(q):
    q = np.asarray(q, np.float64)
    return (q / np.linalg.norm(q)).astype(np.float32)


def poses(seed, W, H):
    """17 seeded poses of objects that fill the screen; the first three are the border cases:
    0: the camera inside the cube (every ray's first sample is the camera itself, clamped cells on the way out);
    1: the camera looks along the object's +x axis: rays that miss leave through the face x = R - 1;
    2: the camera looks along -x: rays ENTER through x = R - 1, so their first sample lies on that face, its cell is
       the clamped one at x = R - 2 and its second record the last x-plane of the array."""
    pos, quat, isc = oracle.random_poses(VIEWS, seed=seed, width=W, height=H, f=0.75 * W)
    pos[0], quat[0], isc[0] = (0.04, -0.03, -0.3), unit((0.1, 0.2, -0.1, 0.95)), 2.0
    pos[1], quat[1], isc[1] = (0.02, 0.01, -1.3), unit((0.04, 0.7071, 0.03, 0.7071)), 2.0
    pos[2], quat[2], isc[2] = (-0.02, 0.03, -1.3), unit((0.03, -0.7071, 0.05, 0.7071)), 2.0
    return pos, quat, isc


def field(kind, Rn):
    return oracle.sphere_sdf(0.5, R=Rn) if kind == "sphere" else oracle.blobs_sdf(0, R=Rn)


def forward(R, sdf, pos, quat, isc, cam, thr):
    return R.forward_raw(sdf, dev(pos), dev(quat), dev(isc), *cam, thr)


@pytest.mark.parametrize("Rn", RESOLUTIONS)
@pytest.mark.parametrize("kind", ["sphere", "blobs"])
def test_packed_depth_equals_plain_grid_depth(R, kind, Rn):
    sdf = dev(field(kind, Rn))
    thr = 0.01
    for W, H in SIZES:
        pos, quat, isc = poses(100 + Rn, W, H)
        cam = (W, H, W / 2.0, H / 2.0, 0.75 * W, 0.75 * W)
        packed = forward(R, sdf, pos, quat, isc, cam, thr)
        plain = torch.cat([forward(R, sdf, pos[s], quat[s], isc[s], cam, thr)
                           for s in (slice(0, 9), slice(9, VIEWS))])
        assert torch.equal(packed, plain), (kind, Rn, W, H, int((packed != plain).sum()))
        hits = (packed > 0).reshape(VIEWS, -1).sum(1)
        # the marches did run (view 0 of the blobs may start inside one: a hit at t = 0 is depth 0)
        assert int(hits[1:3].min()) > 0 and int(hits.sum()) > 20 * VIEWS, hits.tolist()
        assert kind != "sphere" or int(hits[0]) > 0


def test_border_rays_sample_the_last_x_plane():
    """The border poses do what their description says (host arithmetic only: the rays of pose 2 start on the face
    x = R - 1, those of pose 1 that miss the object end there)."""
    W, H = SIZES[0]
    pos, quat, isc = poses(164, W, H)
    for b, sign in ((1, 1.0), (2, -1.0)):
        x, y, z, w = (float(v) for v in quat[b])
        # first column of R^T applied to the viewing direction (0, 0, -1): the object-frame x component of the ray
        dx = -(2.0 * (x * z - w * y))
        assert sign * dx > 0.95, (b, dx)
    assert np.linalg.norm(pos[0]) < 1.0 / isc[0]     # camera inside the cube's inscribed sphere


def test_step_path_against_the_oracle(R):
    """sdfr_render_step_forward + backward of 17 views at R = 16 (the packed march, integer index path), 64 x 48."""
    Rn, W, H = 16, 64, 48
    sdf = field("blobs", Rn)
    pos, quat, isc = poses(7, W, H)
    cam = (W, H, W / 2.0, H / 2.0, 0.75 * W, 0.75 * W)
    args = (dev(sdf), dev(pos), dev(quat), dev(isc))
    depth, state = R.step_forward_raw(*args, *cam, 0.01)
    assert torch.equal(depth, torch.cat([forward(R, args[0], pos[s], quat[s], isc[s], cam, 0.01)
                                         for s in (slice(0, 9), slice(9, VIEWS))]))
    d = depth.cpu().numpy()
    assert (d > 0).sum() > 100 * VIEWS
    g = np.random.default_rng(16).uniform(-1, 1, d.shape).astype(np.float32)
    hb = [t.cpu().numpy() for t in R.step_backward_raw(state, dev(g), depth, *args, *cam)]
    ob = oracle.render_backward(g, d, sdf, pos, quat, isc, *cam[2:], dtype=np.float32)
    assert rel_err(hb[0], ob[0]) <= REL
    pose = np.concatenate([hb[1], hb[2], hb[3][:, None]], axis=1)
    ref = np.concatenate([ob[1], ob[2], ob[3][:, None]], axis=1)
    dimg = oracle.render_derivative_images(d, sdf, pos, quat, isc, *cam[2:], dtype=np.float32)
    l1 = np.abs(dimg * g[..., None]).sum(axis=(1, 2), dtype=np.float64)
    assert np.all(np.abs(pose - ref) <= REL * l1), np.max(np.abs(pose - ref) / l1)
