"""GPU: the resident depth buffer of BatchRenderPlan.forward (sdfr_render_forward_resident /
sdfr_render_step_forward_resident, include/sdfr.h): a culled forward tile stores its zeros only where the previous
forward into the same buffer may have left something.

The reference of every comparison is a FRESH plan whose depth buffer was pre-filled with NaN, so a pixel that the
resident plan wrongly left alone (stale depth of an earlier call) or that nobody ever wrote shows as a difference:
depth is compared with torch.equal over the whole batch, vacated regions included.  Two shapes, so that both tile
forms run: (256, 200x136, f = 300) macro tiles behind the one-launch prologue, (18, 320x240, f = 160) small tiles over
packed records; one ragged image (20, 150x100: no multiple of a tile, no 16-byte rows) in the moving-object case."""
import numpy as np
import pytest
import torch

import oracle
from helpers import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(256, 200, 136, 300.0), (18, 320, 240, 160.0)]
THR = 0.005
_grids = {}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def grid(k):
    """three grids with different may-hit boxes (as tests/test_render_step_gpu.py uses them)"""
    if k not in _grids:
        _grids[k] = dev([oracle.blobs_sdf(0), oracle.blobs_sdf(1), oracle.blobs_sdf(0) + 0.08][k])
    return _grids[k]


def new_plan(B, W, H, f):
    from sdfest_amd import BatchRenderPlan, Camera
    plan = BatchRenderPlan(64, B, Camera(W, H, f, f, W / 2.0, H / 2.0, pixel_center=0.5))
    plan.depth.fill_(float("nan"))
    return plan


def image_gradient(B, W, H):
    return torch.rand((B, H, W), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) * 2 - 1


def reference(shape, sdf, pose, g=None):
    """a fresh plan, NaN in its depth buffer: the plain forward, or the step with its gradients"""
    plan = new_plan(*shape)
    if g is None:
        return plan.forward(sdf, *pose, THR).clone(), None
    d = plan.forward(sdf, *pose, THR, prepare_backward=True).clone()
    return d, [o.clone() for o in plan.backward(g, sdf, *pose)]


def assert_equal(got, ref, name):
    (d, grads), (d0, grads0) = got, ref
    assert not torch.isnan(d0).any(), name
    assert torch.equal(d, d0), f"{name}: {(d != d0).sum().item()} pixels differ"
    if grads0 is not None:
        # the tolerances of test_render_step_gpu.assert_same: pose sums are fixed-order sums of the same tile partials,
        # d/dSDF differs by the order of its float atomics
        (gs, gp, gq, gi), (gs0, gp0, gq0, gi0) = grads, grads0
        for a, b in ((gp, gp0), (gq, gq0), (gi, gi0)):
            assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= 2e-5, name
        assert rel_err(gs.cpu().numpy(), gs0.cpu().numpy()) <= 1e-5, name


def run(plan, sdf, pose, g=None, out=None):
    if g is None:
        return plan.forward(sdf, *pose, THR, out=out).clone(), None
    d = plan.forward(sdf, *pose, THR, prepare_backward=True).clone()
    return d, [o.clone() for o in plan.backward(g, sdf, *pose)]


def moving_poses(B, W, H, f):
    """the object left -> right -> larger -> off screen (all views) -> back -> left again"""
    pos, quat, isc = oracle.random_poses(B, seed=41, width=W, height=H, f=f)
    isc = isc * 2.0                                     # half the benchmark's size: room to move inside the image
    shift = np.zeros_like(pos)
    shift[:, 0] = 0.3 * np.abs(pos[:, 2])
    away = np.zeros_like(pos)
    away[:, 0] = 100.0
    seq = [(pos - shift, isc), (pos + shift, isc), (pos + shift, isc * 0.6), (pos + away, isc), (pos, isc),
           (pos - shift, isc)]
    return [(dev(p), dev(quat), dev(s)) for p, s in seq]


@pytest.mark.parametrize("step", [True, False], ids=["step", "plain"])
@pytest.mark.parametrize("shape", SHAPES + [(20, 150, 100, 120.0)], ids=lambda s: f"B{s[0]}_{s[1]}x{s[2]}")
def test_moving_object(shape, step):
    B, W, H, f = shape
    plan, g, sdf = new_plan(*shape), image_gradient(B, W, H) if step else None, grid(0)
    hits = []
    for k, pose in enumerate(moving_poses(B, W, H, f)):
        assert (plan._resident is not None) == (k > 0)          # every call but the first vouches for the buffer
        got = run(plan, sdf, pose, g)
        assert_equal(got, reference(shape, sdf, pose, g), f"call {k}")
        hits.append(int((got[0] > 0).sum().item()))
    assert hits[3] == 0 and min(hits[:3] + hits[4:]) > 100 * B / 20, hits


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}_{s[1]}x{s[2]}")
def test_changing_grid_at_fixed_poses(shape):
    B, W, H, f = shape
    pose = tuple(dev(a) for a in oracle.random_poses(B, seed=11, width=W, height=H, f=f))
    plan, g = new_plan(*shape), image_gradient(B, W, H)
    for k in range(6):
        sdf = grid(k % 3)
        assert_equal(run(plan, sdf, pose, g), reference(shape, sdf, pose, g), f"step {k}")
        assert plan._resident is not None


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}_{s[1]}x{s[2]}")
def test_views_without_valid_spans_and_the_prologue_fallback(shape):
    """Views whose cube has a corner behind the camera (or the camera inside it) have no band spans: their rectangle
    is the whole image.  And one call of the sequence takes the prologue's fall-back path (whole cube as the may-hit
    box), forced through the workspace's poll bound -- written through `.data`, so that the plan still vouches."""
    from sdfest_amd import _lib
    B, W, H, f = shape
    pos, quat, isc = oracle.random_poses(B, seed=43, width=W, height=H, f=f)
    isc = isc * 2.0
    inside = pos.copy()
    inside[0] = (0.0, 0.0, -0.1)                        # the camera inside the cube
    inside[1] = (0.0, 0.0, -0.3)                        # corners behind the camera
    moved = pos.copy()
    moved[:, 0] += 0.2 * np.abs(pos[:, 2])
    normal, odd, other = ((dev(p), dev(quat), dev(isc)) for p in (pos, inside, moved))
    plan, sdf = new_plan(*shape), grid(0)
    o = _lib.lib().sdfr_render_sync_offset(B)
    polls = plan.workspace.data[o + 24:o + 32].view(torch.int32)
    before = plan.prologue_fallbacks()
    for k, pose in enumerate([normal, odd, normal, other, normal, other]):
        if k == 3:
            polls.copy_(torch.tensor([_lib.ABI["SDFR_SYNC_POLLS_MAGIC"], 0], dtype=torch.int64).to(torch.int32))
        assert (plan._resident is not None) == (k > 0)
        got = run(plan, sdf, pose)
        if k == 3:
            polls.zero_()
            assert plan.prologue_fallbacks() - before == B
        assert_equal(got, reference(shape, sdf, pose), f"call {k}")


def corner_free_poses(B, W, H, f):
    """small objects in the right half of the image: the tiles of the image's first columns are never live"""
    _, quat, _ = oracle.random_poses(B, seed=44, width=W, height=H, f=f)
    z = 1.5
    pos = np.tile(np.array([[0.25 * W * z / f, 0.0, -z]], dtype=np.float32), (B, 1))
    return dev(pos), dev(quat), dev(np.full(B, 10.0, dtype=np.float32))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}_{s[1]}x{s[2]}")
def test_it_is_really_skipping(shape):
    B, W, H, f = shape
    pose, sdf = corner_free_poses(B, W, H, f), grid(0)
    ref = reference(shape, sdf, pose)[0]
    assert (ref > 0).sum().item() > 20 * B and (ref[:, :, :32] == 0).all()
    plan = new_plan(*shape)
    assert torch.equal(plan.forward(sdf, *pose, THR), ref)
    plan.depth.data[:, 0, 0] = 7.0                       # through .data: torch's version counter does not see it
    d = plan.forward(sdf, *pose, THR)
    assert (d[:, 0, 0] == 7.0).all(), "the culled corner tiles were stored again"
    d[:, 0, 0] = 0.0
    assert torch.equal(d, ref)
    plan.depth[:, 0, 0] = 7.0                            # an in-place write torch knows of: one full fill
    assert torch.equal(plan.forward(sdf, *pose, THR), ref)


def test_sixteen_views_always_store_every_pixel():
    """below 17 views the plain grid is marched and the set-up has no band spans: the feature is off"""
    shape = (16, 320, 240, 160.0)
    pose, sdf = corner_free_poses(*shape), grid(0)
    ref = reference(shape, sdf, pose)[0]
    plan = new_plan(*shape)
    for _ in range(3):
        assert torch.equal(plan.forward(sdf, *pose, THR), ref)
        plan.depth.data[:, 0, 0] = 7.0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}_{s[1]}x{s[2]}")
def test_invalidation(shape):
    B, W, H, f = shape
    poses, sdf, g = moving_poses(B, W, H, f), grid(0), image_gradient(B, W, H)
    refs = [reference(shape, sdf, p)[0] for p in poses[:3]]
    # out= alternating between two buffers
    plan = new_plan(*shape)
    bufs = [torch.full_like(plan.depth, float("nan")) for _ in range(2)]
    for k in (0, 1, 2, 0, 1, 2, 2):
        buf = bufs[k % 2] if k != 2 else bufs[0]
        assert torch.equal(plan.forward(sdf, *poses[k], THR, out=buf), refs[k]), f"out= call with pose {k}"
    # a forward_l1 / a stand-alone backward between two forwards
    plan = new_plan(*shape)
    assert torch.equal(plan.forward(sdf, *poses[0], THR), refs[0])
    plan.forward_l1(sdf, *poses[1], THR, refs[1])
    assert plan._resident is None
    assert torch.equal(plan.forward(sdf, *poses[2], THR), refs[2])
    plan.backward(g, sdf, *poses[2])
    assert plan._resident is None
    assert torch.equal(plan.forward(sdf, *poses[0], THR), refs[0])
    # the workspace overwritten between two forwards
    gen = torch.Generator(device="cuda").manual_seed(5)
    for k, fill in enumerate(("ones", "random", "ones")):
        if fill == "ones":
            plan.workspace.fill_(255)
        else:
            plan.workspace.copy_(torch.randint(0, 256, plan.workspace.shape, device="cuda", generator=gen,
                                               dtype=torch.uint8))
        assert torch.equal(plan.forward(sdf, *poses[1 + k % 2], THR), refs[1 + k % 2]), fill
    # ... and the state itself: whatever it holds, a call that does not vouch stores every pixel and rewrites it
    plan.ring_reset()
    plan._resident_state.copy_(torch.randint(0, 256, plan._resident_state.shape, device="cuda", generator=gen,
                                             dtype=torch.uint8))
    assert torch.equal(plan.forward(sdf, *poses[0], THR), refs[0])
    assert torch.equal(plan.forward(sdf, *poses[1], THR), refs[1])


def test_a_foreign_state_never_validates():
    """The C ABI directly: the caller vouches (depth_resident = 1) but hands over a state that no previous call wrote
    -- zeros, ones, random bytes, another shape's state: no row validates and every pixel is stored."""
    from sdfest_amd import _lib
    from sdfest_amd.differentiable_renderer import _stream
    shape = (18, 320, 240, 160.0)
    B, W, H, f = shape
    L = _lib.lib()
    pose, sdf = corner_free_poses(*shape), grid(0)
    ref = reference(shape, sdf, pose)[0]
    plan = new_plan(*shape)
    other = new_plan(20, 320, 240, 160.0)
    other.forward(sdf, *corner_free_poses(20, 320, 240, 160.0), THR)
    n = L.sdfr_render_resident_state_bytes(B, H)
    gen = torch.Generator(device="cuda").manual_seed(6)
    states = [torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.full((n,), 255, dtype=torch.uint8, device="cuda"),
              torch.randint(0, 256, (n,), device="cuda", generator=gen, dtype=torch.uint8),
              other._resident_state[:n].clone()]
    for k, state in enumerate(states):
        depth = torch.full_like(plan.depth, float("nan"))
        rc = L.sdfr_render_forward_resident(sdf.data_ptr(), 64, 0, pose[0].data_ptr(), pose[1].data_ptr(),
                                            pose[2].data_ptr(), B, W, H, W / 2.0, H / 2.0, f, f, THR, depth.data_ptr(),
                                            plan.workspace.data_ptr(), plan.workspace.numel(), state.data_ptr(),
                                            state.numel(), 1, plan.device.index, _stream(plan.device))
        _lib.check(rc, "sdfr_render_forward_resident")
        assert torch.equal(depth, ref), f"state {k}"
    rc = L.sdfr_render_forward_resident(sdf.data_ptr(), 64, 0, pose[0].data_ptr(), pose[1].data_ptr(),
                                        pose[2].data_ptr(), B, W, H, W / 2.0, H / 2.0, f, f, THR, plan.depth.data_ptr(),
                                        plan.workspace.data_ptr(), plan.workspace.numel(), states[0].data_ptr(), 64, 1,
                                        plan.device.index, _stream(plan.device))
    assert rc == _lib.ABI["SDFR_E_WORKSPACE"] and b"resident state" in L.sdfr_last_error()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}_{s[1]}x{s[2]}")
def test_graph_replay(shape):
    """A captured step vouches with the SAME kernel arguments in every replay: what the previous replay left is
    handed over on the device.  New poses and a new grid are copied into the captured tensors between replays."""
    B, W, H, f = shape
    poses, g = moving_poses(B, W, H, f), image_gradient(B, W, H)
    sdf = grid(0).clone()
    pose = tuple(t.clone() for t in poses[4])
    plan = new_plan(*shape)
    run(plan, sdf, pose, g)
    run(plan, sdf, pose, g)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            d = plan.forward(sdf, *pose, THR, prepare_backward=True)
            grads = plan.backward(g, sdf, *pose)
    for k, p in enumerate([poses[0], poses[1], poses[3], poses[2], poses[5]]):
        for dst, src in zip(pose, p):
            dst.copy_(src)
        sdf.copy_(grid(k % 3))
        graph.replay()
        torch.cuda.synchronize()
        assert_equal((d, grads), reference(shape, sdf, pose, g), f"replay {k}")
