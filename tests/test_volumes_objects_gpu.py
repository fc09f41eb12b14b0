"""GPU, C ABI: sdfr_volumes_replicate (K volumes -> K V, one per view) and sdfr_volumes_sum_views (K V gradient volumes
-> K, summed per object in a fixed order) -- the two copies a K-object loop with V views per object adds to an iteration.

R = 8: rows of 512 floats, every one on a 16-byte boundary (the 16-byte path and nothing else); R = 9: rows of 729
floats, three rows in four start off the boundary and every row ends in a single float (the scalar path, the vector
path's scalar end, and a workgroup whose last threads have nothing to do).  R = 17: 4913 floats, more than one
workgroup per row.  Both results are exact: a copy, and one order of fp32 additions."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [(2, 3, 8), (2, 3, 9), (3, 1, 9), (2, 3, 17), (1, 4, 8)]


def call(name, src, dst, K, V, n):
    from sdfest_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(src.data_ptr(), dst.data_ptr(), K, V, n, 0,
                                         torch.cuda.current_stream().cuda_stream), name)


def guarded(rows, n):
    """rows x n floats between two guard floats -- on a 16-byte boundary itself, like every buffer of the loop"""
    buf = torch.full((rows * n + 8,), 777.0, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[4:4 + rows * n].view(rows, n)


@pytest.mark.parametrize("K,V,R", CASES)
def test_replicate_is_a_bit_copy(K, V, R):
    n = R ** 3
    rng = np.random.default_rng(R + V)
    src_np = rng.normal(size=(K, n)).astype(np.float32)
    src_np[0, :4] = [np.nan, np.inf, -0.0, 1e-42]          # bits, not values
    src = torch.tensor(src_np, device="cuda")
    buf, dst = guarded(K * V, n)
    call("sdfr_volumes_replicate", src, dst, K, V, n)
    torch.cuda.synchronize()
    want = np.repeat(src_np, V, axis=0)                    # row k V + v = row k
    assert np.array_equal(dst.cpu().numpy().view(np.int32), want.view(np.int32))
    assert torch.all(buf[:4] == 777.0) and torch.all(buf[-4:] == 777.0)
    assert np.array_equal(src.cpu().numpy().view(np.int32), src_np.view(np.int32))


@pytest.mark.parametrize("K,V,R", CASES)
def test_sum_views_is_the_fp32_sum_in_view_order_on_every_run(K, V, R):
    n = R ** 3
    rng = np.random.default_rng(10 * R + V)
    # magnitudes spread over six decades: another order of additions would round differently
    src_np = (rng.normal(size=(K * V, n)) * 10.0 ** rng.uniform(-3, 3, size=(K * V, n))).astype(np.float32)
    src = torch.tensor(src_np, device="cuda")
    want = src_np.reshape(K, V, n)[:, 0].copy()
    for v in range(1, V):
        want = want + src_np.reshape(K, V, n)[:, v]        # ((s0 + s1) + s2) + ..., float32 throughout
    assert want.dtype == np.float32
    if V > 2:    # (the order matters for this data, so the comparison below says something about it)
        other = src_np.reshape(K, V, n)[:, 0] + (src_np.reshape(K, V, n)[:, 1] + src_np.reshape(K, V, n)[:, 2])
        for v in range(3, V):
            other = other + src_np.reshape(K, V, n)[:, v]
        assert not np.array_equal(other, want)
    outs = []
    for run in range(2):
        buf, dst = guarded(K, n)
        call("sdfr_volumes_sum_views", src, dst, K, V, n)
        torch.cuda.synchronize()
        assert torch.all(buf[:4] == 777.0) and torch.all(buf[-4:] == 777.0)
        outs.append(dst.cpu().numpy().copy())
    assert np.array_equal(outs[0].view(np.int32), want.view(np.int32))
    assert np.array_equal(outs[1].view(np.int32), outs[0].view(np.int32))
