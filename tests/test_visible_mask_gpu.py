"""GPU: ``sdfr_visible_mask`` / ``mesh.visible_mask`` -- the reference's ``_compute_mask`` (redwood_dataset.py:262-275)
for B images -- against the torch expression ``(r != 0) & ~((o != 0) & (o < r - margin))`` on the same device, exactly:
every pixel class (nothing rendered, no reading under cover, a reading exactly at the margin, one ulp in front of it,
far in front, behind, infinite, NaN), image sizes that are no multiple of 4 (image 1 starts unaligned), views one and
two floats into a larger buffer (the 16-byte and the pixel-by-pixel form), more than one workgroup per image."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 7), (2, 3, 64), (2, 120, 160), (1, 480, 640)]
CLASSES = 8


def images(shape, margin, offset_r=0, offset_o=0, seed=0):
    """(rendered, observed) of `shape`, each a view `offset` floats into a larger buffer; the pixels cycle through
    the classes, shifted by one from image to image"""
    B, H, W = shape
    n = B * H * W
    gen = torch.Generator(device="cuda").manual_seed(seed)
    r = torch.rand(n, generator=gen, device="cuda") * 1.2 + 0.3
    cls = (torch.arange(n, device="cuda") + torch.arange(B, device="cuda").repeat_interleave(H * W)) % CLASSES
    edge = r - margin                                   # fl(rendered - margin), as the kernel forms it
    o = torch.empty_like(r)
    o[cls == 0] = 0.7                                   # nothing rendered there (rendered set to 0 below)
    o[cls == 1] = 0.0                                   # no reading under cover
    o[cls == 2] = edge[cls == 2]                        # exactly at the margin: the comparison is strict
    o[cls == 3] = torch.nextafter(edge, torch.full_like(edge, -1.0))[cls == 3]      # one ulp in front of it
    o[cls == 4] = (0.5 * r)[cls == 4]                   # far in front
    o[cls == 5] = (r + 0.3)[cls == 5]                   # behind
    o[cls == 6] = float("inf")
    o[cls == 7] = float("nan")
    r[cls == 0] = 0.0
    buf_r = torch.full((n + 8,), -1.0, device="cuda")
    buf_o = torch.full((n + 8,), -1.0, device="cuda")
    buf_r[offset_r:offset_r + n] = r
    buf_o[offset_o:offset_o + n] = o
    rv, ov = buf_r[offset_r:offset_r + n].view(B, H, W), buf_o[offset_o:offset_o + n].view(B, H, W)
    assert rv.is_contiguous() and rv.data_ptr() == buf_r.data_ptr() + 4 * offset_r
    return rv, ov, cls.view(B, H, W)


def expected(r, o, margin):
    mask = (r != 0) & ~((o != 0) & (o < r - margin))
    masked = torch.where(mask, o, torch.zeros_like(o))
    covered = r != 0
    counts = torch.stack([covered.flatten(1).sum(1), mask.flatten(1).sum(1), (covered & ~mask).flatten(1).sum(1),
                          (mask & (o != 0)).flatten(1).sum(1)], 1).to(torch.int32)
    return mask, masked, counts


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))       # (NaN pixels compare as their bits)


CASES = [(s, 0, 0) for s in SHAPES] + [((3, 5, 7), 1, 1), ((3, 5, 7), 1, 2), ((2, 3, 64), 3, 3)]


@pytest.mark.parametrize("margin", [0.0, 0.01])
@pytest.mark.parametrize("shape, offset_r, offset_o", CASES,
                         ids=[f"{s[0]}x{s[1]}x{s[2]}+{a}+{b}" for s, a, b in CASES])
def test_mask_masked_and_counts_equal_the_torch_expression(shape, offset_r, offset_o, margin):
    from sdfest_amd import visible_mask
    r, o, cls = images(shape, margin, offset_r, offset_o)
    want_mask, want_masked, want_counts = expected(r, o, margin)
    mask, masked, counts = visible_mask(r, o, margin, return_masked=True, return_counts=True)
    torch.cuda.synchronize()
    assert mask.dtype == torch.bool and mask.shape == r.shape and masked.dtype == torch.float32
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (shape[0], 4)
    assert torch.equal(mask.view(torch.uint8), want_mask.view(torch.uint8))      # bytes of 0 and 1
    assert same_bits(masked, want_masked)
    assert torch.equal(counts, want_counts)
    # what each class must give, whatever torch says
    for c, visible in ((0, False), (1, True), (2, True), (3, False), (4, False), (5, True), (6, True), (7, True)):
        if (cls == c).any():
            assert bool((mask[cls == c] == visible).all()), c
    # the mask alone, and a single (H,W) image
    assert torch.equal(visible_mask(r, o, margin), mask)
    one = visible_mask(r[-1], o[-1], margin, return_counts=True)
    assert torch.equal(one[0], mask[-1]) and torch.equal(one[1], counts[-1])


def raw_call(r, o, margin, mask, masked, counts):
    from sdfest_amd import _lib
    B, H, W = r.shape
    _lib.check(_lib.lib().sdfr_visible_mask(r.data_ptr(), o.data_ptr(), B, H, W, margin, mask.data_ptr(),
                                            masked.data_ptr(), counts.data_ptr(), r.device.index,
                                            torch.cuda.current_stream().cuda_stream), "sdfr_visible_mask")


def test_a_second_call_overwrites_and_a_captured_graph_replays():
    shape, margin = (3, 5, 7), 0.01
    r, o, _ = images(shape, margin)
    want_mask, want_masked, want_counts = expected(r, o, margin)
    mask = torch.empty(shape, dtype=torch.bool, device="cuda")
    masked = torch.full(shape, 7.0, device="cuda")
    counts = torch.full((shape[0], 4), 1000, dtype=torch.int32, device="cuda")      # overwritten, not added to
    for _ in range(2):
        raw_call(r, o, margin, mask, masked, counts)
        torch.cuda.synchronize()
        assert torch.equal(mask, want_mask) and same_bits(masked, want_masked) and torch.equal(counts, want_counts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        raw_call(r, o, margin, mask, masked, counts)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_call(r, o, margin, mask, masked, counts)
    # other images written in place, one replay
    r2, o2, _ = images(shape, margin, seed=3)
    r.copy_(r2.roll(1, 0)), o.copy_(o2.roll(1, 0))
    want_mask, want_masked, want_counts = expected(r, o, margin)
    mask.fill_(True), masked.fill_(5.0), counts.fill_(-3)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(mask, want_mask) and same_bits(masked, want_masked) and torch.equal(counts, want_counts)


def test_python_front_refuses_bad_arguments():
    from sdfest_amd import visible_mask
    r = torch.zeros((2, 4, 4), device="cuda")
    with pytest.raises(ValueError):
        visible_mask(r, r, margin=-1.0)
    with pytest.raises(ValueError):
        visible_mask(r, r, margin=float("nan"))
    with pytest.raises(TypeError):
        visible_mask(r.double(), r.double())
    empty = visible_mask(r[:0], r[:0], return_counts=True)
    assert tuple(empty[0].shape) == (0, 4, 4) and tuple(empty[1].shape) == (0, 4)
