"""GPU: the resident grid of BatchRenderPlan.forward (sdfr_render_forward_grid_resident /
sdfr_render_step_forward_grid_resident, include/sdfr.h): a forward on the grid its predecessor packed neither packs nor
reduces the plane minima again.

The reference of every comparison is a FRESH plan (``grid_resident=False``: it never vouches), and everything is compared
bit for bit: depth, the pose gradients, and d/dSDF in the deterministic mode.  Shapes: the smallest that take the packed
path -- (R, B) = (16, 17) and (32, 18), 64 x 48 pixels -- and R = 18 for the two-launch form (R % 4 != 0)."""
import ctypes

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

W, H, F = 64, 48, 32.0
SHAPES = [(16, 17), (32, 18), (18, 17)]
IDS = [f"R{r}_B{b}" for r, b in SHAPES]
GRID_MAGIC = 0x47524944
_cache = {}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def grid_np(R, k=0):
    if (R, k) not in _cache:
        _cache[(R, k)] = oracle.blobs_sdf(k, R=R)
    return _cache[(R, k)]


def poses(B, seed):
    return tuple(dev(a) for a in oracle.random_poses(B, seed=seed, width=W, height=H, f=F))


def image_gradient(B):
    return torch.rand((B, H, W), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) * 2 - 1


def new_plan(R, B, grid_resident="auto"):
    from sdfest_amd import BatchRenderPlan, Camera
    from sdfest_amd.differentiable_renderer import SDF_GRAD_DETERMINISTIC, SDF_GRAD_EXACT
    plan = BatchRenderPlan(R, B, Camera(W, H, F, F, W / 2.0, H / 2.0, pixel_center=0.5),
                           sdf_grad_mode=SDF_GRAD_EXACT | SDF_GRAD_DETERMINISTIC, grid_resident=grid_resident)
    plan.grid_verify = True
    return plan


def step(plan, sdf, pose, thr, g):
    d = plan.forward(sdf, *pose, thr, prepare_backward=True).clone()
    flag = plan.grid_flag
    return [d] + [o.clone() for o in plan.backward(g, sdf, *pose)], flag


def fresh(R, B, sdf, pose, thr, g=None):
    plan = new_plan(R, B, grid_resident=False)
    if g is None:
        return [plan.forward(sdf, *pose, thr).clone()]
    out, flag = step(plan, sdf, pose, thr, g)
    assert flag == 0
    return out


def assert_bitwise(got, ref, name):
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), f"{name}: output {k} differs in {(a != b).sum().item()} elements"
    assert (ref[0] > 0).sum().item() > 20 * ref[0].shape[0], name


def sync_words(plan):
    o = plan._sync_offset
    return plan.workspace[o:o + 128].view(torch.int32).tolist()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_same_grid_new_poses_and_threshold(shape):
    R, B = shape
    from sdfest_amd import _lib
    plan, sdf, g = new_plan(R, B), dev(grid_np(R)), image_gradient(B)
    before = plan.prologue_fallbacks()
    for k, (seed, thr) in enumerate([(1, 0.005), (2, 0.02), (3, 0.011)]):
        pose = poses(B, seed)
        got, flag = step(plan, sdf, pose, thr, g)
        assert flag == (_lib.ABI["SDFR_GRID_RESIDENT_VERIFY"] if k else 0)
        assert_bitwise(got, fresh(R, B, sdf, pose, thr, g), f"call {k}")
    assert plan.grid_mismatches() == 0 and plan.prologue_fallbacks() == before
    words = sync_words(plan)
    assert (words[8], words[9]) == (GRID_MAGIC, R | (1 if R % 4 == 0 else 2) << 16)
    # the plain forward (forward layout of the same workspace: the records have the same place)
    pose = poses(B, 4)
    d = plan.forward(sdf, *pose, 0.005).clone()
    assert plan.grid_flag != 0 and plan.grid_mismatches() == 0
    assert_bitwise([d], fresh(R, B, sdf, pose, 0.005), "plain")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_in_place_update_and_another_tensor_repack(shape):
    R, B = shape
    plan, g, pose = new_plan(R, B), image_gradient(B), poses(B, 5)
    sdf, other = dev(grid_np(R)), dev(grid_np(R, 1))
    assert step(plan, sdf, pose, 0.005, g)[1] == 0
    sdf.mul_(1.01)                                        # the version moves: the plan packs the new bytes
    got, flag = step(plan, sdf, pose, 0.005, g)
    assert flag == 0
    assert_bitwise(got, fresh(R, B, sdf, pose, 0.005, g), "after mul_")
    for k, t in enumerate([other, sdf, other, other]):    # another tensor of the same shape in between
        got, flag = step(plan, t, pose, 0.005, g)
        assert flag == (0 if k < 3 else 2), k
        assert_bitwise(got, fresh(R, B, t, pose, 0.005, g), f"tensor {k}")
    assert plan.grid_mismatches() == 0


def test_a_grid_freed_and_another_in_its_place_is_not_vouched_for():
    R, B = 16, 17
    plan, pose = new_plan(R, B), poses(B, 5)
    sdf = dev(grid_np(R))
    plan.forward(sdf, *pose, 0.005)
    ptr = sdf.data_ptr()
    del sdf
    sdf = dev(grid_np(R, 1))                              # the allocator hands the block out again (if not: no test)
    d = plan.forward(sdf, *pose, 0.005).clone()
    assert plan.grid_flag == 0, (ptr, sdf.data_ptr())
    assert_bitwise([d], fresh(R, B, sdf, pose, 0.005), "reallocated")


@pytest.mark.parametrize("between", ["backward", "forward_l1", "second_plan"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=IDS[:2])
def test_other_calls_on_the_workspace_leave_no_stale_vouch(shape, between):
    R, B = shape
    plan, g, pose = new_plan(R, B), image_gradient(B), poses(B, 6)
    sdf, other = dev(grid_np(R)), dev(grid_np(R, 1))
    plan.forward(sdf, *pose, 0.005)
    if between == "backward":                             # stand-alone: its tile partials lie over the records
        plan.backward(g, sdf, *pose)
    elif between == "forward_l1":                         # packs ANOTHER grid into the same records
        plan.forward_l1(other, *pose, 0.005, g.abs())
    else:                                                 # a second plan that was given the same workspace tensor
        second = new_plan(R, B)
        second.workspace = plan.workspace
        second.forward(other, *pose, 0.005)
        assert second.grid_flag == 0
    d = plan.forward(sdf, *pose, 0.005).clone()
    assert plan.grid_flag == 0
    assert_bitwise([d], fresh(R, B, sdf, pose, 0.005), between)
    d = plan.forward(sdf, *pose, 0.005).clone()           # and now it may
    assert plan.grid_flag != 0 and plan.grid_mismatches() == 0
    assert_bitwise([d], fresh(R, B, sdf, pose, 0.005), between + ", vouched")


def view_records(plan):
    return plan.workspace[:plan.B * 256].view(torch.float32).view(plan.B, 64).clone()


@pytest.mark.parametrize("shape", SHAPES[:2], ids=IDS[:2])
def test_minima_survive_a_call_whose_set_ups_fell_back(shape):
    """The kept minima come from the plane blocks: a packing call with a poll bound of 0 rounds sets every view up
    without them (may-hit box = the cube), and the resident call behind it has them all the same."""
    from sdfest_amd import _lib
    R, B = shape
    plan, sdf, pose = new_plan(R, B), dev(grid_np(R)), poses(B, 8)
    o = plan._sync_offset
    polls = plan.workspace.data[o + 24:o + 32].view(torch.int32)    # (.data: the workspace's version stays)
    polls.copy_(torch.tensor([_lib.ABI["SDFR_SYNC_POLLS_MAGIC"], 0], dtype=torch.int64).to(torch.int32))
    d0 = plan.forward(sdf, *pose, 0.005).clone()
    assert plan.grid_flag == 0 and plan.prologue_fallbacks() == B
    rec0 = view_records(plan)
    polls.zero_()
    d1 = plan.forward(sdf, *pose, 0.005).clone()
    assert plan.grid_flag != 0 and plan.prologue_fallbacks() == B and plan.grid_mismatches() == 0
    rec1 = view_records(plan)
    ref = new_plan(R, B, grid_resident=False)
    d_ref = ref.forward(sdf, *pose, 0.005).clone()
    assert torch.equal(d0, d_ref) and torch.equal(d1, d_ref)
    assert torch.equal(rec1.view(torch.int32)[:, :43], view_records(ref).view(torch.int32)[:, :43])   # (then padding)
    # ViewSetup (common.hpp): rect = words 24..27, cube planes ep / em = 28..33, may-hit planes tp / tm = 35..40
    assert torch.equal(rec0[:, 35:41], rec0[:, 28:34])              # the fall-back: the whole cube
    assert (rec1[:, 35:38] < rec1[:, 28:31]).any() and (rec1[:, 38:41] > rec1[:, 31:34]).any()
    area = lambda r: ((r[:, 26] - r[:, 24]) * (r[:, 27] - r[:, 25]))
    r0, r1 = rec0.view(torch.int32), rec1.view(torch.int32)
    assert (area(r1) <= area(r0)).all() and (area(r1) < area(r0)).any()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bytes_changed_behind_the_version_counter_are_counted(shape):
    """The hazard the option cannot remove: a write through the raw pointer does not move ``_version``, the plan
    vouches, and the march reads the records of the old bytes.  The verification switch counts them;
    ``invalidate_grid()`` is the caller's way out."""
    R, B = shape
    plan, sdf, pose = new_plan(R, B), dev(grid_np(R)), poses(B, 9)
    plan.forward(sdf, *pose, 0.005)
    sdf.data[R // 2, R // 2, R // 2] += 0.25             # no version bump
    d = plan.forward(sdf, *pose, 0.005).clone()
    assert plan.grid_flag != 0
    n = plan.grid_mismatches()
    assert 1 <= n <= 4                                    # the voxel is a corner of up to four face records
    plan.forward(sdf, *pose, 0.005)
    plan.invalidate_grid()
    d = plan.forward(sdf, *pose, 0.005).clone()
    assert plan.grid_flag == 0
    assert_bitwise([d], fresh(R, B, sdf, pose, 0.005), "after invalidate_grid")
    before = plan.grid_mismatches()
    plan.forward(sdf, *pose, 0.005)
    assert plan.grid_flag != 0 and plan.grid_mismatches() == before


def c_forward(R, B, sdf, pose, ws, flag, thr=0.005):
    from sdfest_amd import _lib
    L = _lib.lib()
    depth = torch.full((B, H, W), float("nan"), device="cuda")
    rc = L.sdfr_render_forward_grid_resident(
        sdf.data_ptr(), R, 0, pose[0].data_ptr(), pose[1].data_ptr(), pose[2].data_ptr(), B, W, H, W / 2.0, H / 2.0,
        F, F, thr, depth.data_ptr(), ws.data_ptr(), ws.numel(), None, 0, 0, flag, torch.cuda.current_device(),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.lib().sdfr_last_error()
    return depth


@pytest.mark.parametrize("form", [32, 18], ids=["one_launch", "two_launch"])
def test_c_entry_points_fall_back_to_packing(form):
    from sdfest_amd import _lib
    L, B, R = _lib.lib(), 18, form
    small = R // 2 if form == 32 else 14                  # another R of the same form
    n = max(L.sdfr_render_step_workspace_bytes(R, B, W, H), L.sdfr_render_step_workspace_bytes(small, B, W, H))
    pose = poses(B, 10)
    sdf, sdf_small = dev(grid_np(R)), dev(grid_np(small))
    ref, ref_small = fresh(R, B, sdf, pose, 0.005)[0], fresh(small, B, sdf_small, pose, 0.005)[0]
    for fill in (0, 0xA5):                                # a workspace that never packed: zeros, or foreign bytes
        ws = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
        assert torch.equal(c_forward(R, B, sdf, pose, ws, 1), ref)
        o = L.sdfr_render_sync_offset(B)
        assert ws[o + 32:o + 40].view(torch.int32).tolist() == [GRID_MAGIC, R | (1 if R % 4 == 0 else 2) << 16]
        assert torch.equal(c_forward(R, B, sdf, pose, ws, 2), ref)          # resident now, and verified
        assert torch.equal(c_forward(small, B, sdf_small, pose, ws, 1), ref_small)   # another R: packs
        assert torch.equal(c_forward(small, B, sdf_small, pose, ws, 2), ref_small)
        assert torch.equal(c_forward(R, B, sdf, pose, ws, 1), ref)          # and back
        word = o + 4 * _lib.ABI["SDFR_SYNC_GRID_MISMATCH_WORD"]
        assert ws[word:word + 4].view(torch.int32).item() == (0 if fill == 0 else 0xA5A5A5A5 - 2 ** 32)   # untouched


def test_step_entry_point_and_a_call_with_few_views_ignore_the_flag():
    from sdfest_amd import _lib
    L, R = _lib.lib(), 16
    for B in (16, 17):                                    # 16 views: no packed grid, the flag means nothing
        pose, sdf = poses(B, 11), dev(grid_np(R))
        ws = torch.zeros(L.sdfr_render_step_workspace_bytes(R, B, W, H), dtype=torch.uint8, device="cuda")
        ref = fresh(R, B, sdf, pose, 0.005)[0]
        for _ in range(2):
            depth = torch.full((B, H, W), float("nan"), device="cuda")
            g_sdf = torch.full((R, R, R), float("nan"), device="cuda")
            rc = L.sdfr_render_step_forward_grid_resident(
                sdf.data_ptr(), R, 0, pose[0].data_ptr(), pose[1].data_ptr(), pose[2].data_ptr(), B, W, H, W / 2.0,
                H / 2.0, F, F, 0.005, depth.data_ptr(), g_sdf.data_ptr(), 0, ws.data_ptr(), ws.numel(), None, None, 0,
                0, 2, torch.cuda.current_device(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
            assert torch.equal(depth, ref) and not g_sdf.any()      # the zero fill happens in both forms
        o = L.sdfr_render_sync_offset(B)
        assert ws[o + 32:o + 36].view(torch.int32).item() == (GRID_MAGIC if B == 17 else 0)
        assert ws[o + 44:o + 48].view(torch.int32).item() == 0


def test_no_vouch_while_the_stream_is_capturing():
    R, B = 16, 17
    plan, sdf, pose = new_plan(R, B), dev(grid_np(R)), poses(B, 12)
    plan.forward(sdf, *pose, 0.005)
    plan.forward(sdf, *pose, 0.005)
    assert plan.grid_flag != 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.forward(sdf, *pose, 0.005)
        assert plan.grid_flag == 0
        plan.forward(sdf, *pose, 0.005)
        assert plan.grid_flag == 0                        # a captured forward leaves nothing to vouch for either
    plan.forward(sdf, *pose, 0.005)
    assert plan.grid_flag == 0                            # nor does the capture: what a replay packs, nobody saw
    d = plan.forward(sdf, *pose, 0.005).clone()
    assert plan.grid_flag != 0
    assert_bitwise([d], fresh(R, B, sdf, pose, 0.005), "after the capture")
