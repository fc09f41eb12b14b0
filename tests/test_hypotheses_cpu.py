"""CPU: the orientation-hypothesis entry points (``sdfr_orientation_topk``, ``sdfr_init_hypotheses``, ``sdfr_select_row``)
are declared, exported and bound; they refuse bad arguments before any HIP call; and the numpy twin the GPU tests
compare against (tests/hypotheses_twin.py) gives the hand-written answers of its three rules."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import hypotheses_twin as twin

NAMES = ("sdfr_orientation_topk", "sdfr_init_hypotheses", "sdfr_select_row")


@pytest.fixture(scope="module")
def L():
    from sdfest_amd import _lib
    _lib.build()
    return _lib.lib()


def test_the_three_symbols_are_declared_bound_and_exported(L):
    from sdfest_amd import _lib
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["sdfr_orientation_topk"] == (i, [vp, i, i, vp, vp, i, vp])
    assert _lib.SIGNATURES["sdfr_init_hypotheses"] == (i, [vp, i, vp, i, vp, i, vp, vp, i, vp])
    assert _lib.SIGNATURES["sdfr_select_row"] == (i, [vp, i, i, vp, i, vp, vp, vp, i, vp])
    assert _lib.ABI["SDFR_MAX_HYPOTHESES"] == twin.MAX_HYPOTHESES == 32
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.sdfr_version() == 100
    # the header's CONTENTS comment lists them under their groups: 4, 4 and 3
    text = open(_lib.HEADER).read()
    contents = text[text.index("CONTENTS"):text.index("#ifndef SDFR_H_")]
    g3, g4, g5 = contents.index("3. [unstable] LOOP"), contents.index("4. [unstable] GENERATOR"), contents.index("5. [unstable]")
    assert g3 < contents.index("sdfr_select_row") < g4
    assert g4 < contents.index("sdfr_orientation_topk") < g5 and g4 < contents.index("sdfr_init_hypotheses") < g5


def test_argument_errors_without_gpu(L):
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)     # a non-NULL pointer that is never dereferenced
    err = lambda: L.sdfr_last_error()
    # sdfr_orientation_topk(posterior, C, N, out_index, out_prob, device, stream)
    assert L.sdfr_orientation_topk(q, 576, 0, q, q, 0, None) == -1 and b"N=0" in err()
    assert L.sdfr_orientation_topk(q, 576, 33, q, q, 0, None) == -1 and b"N=33" in err()
    assert L.sdfr_orientation_topk(q, 4, 5, q, q, 0, None) == -1 and b"C=4" in err()
    assert L.sdfr_orientation_topk(q, (1 << 24) + 1, 5, q, q, 0, None) == -1
    assert L.sdfr_orientation_topk(None, 576, 4, q, q, 0, None) == -2 and b"sdfr_orientation_topk: NULL" in err()
    assert L.sdfr_orientation_topk(q, 576, 4, None, q, 0, None) == -2
    assert L.sdfr_orientation_topk(q, 576, 4, q, None, 0, None) == -2
    # sdfr_init_hypotheses(params_one, n_params, grid_quats, C, index, N, cam_quat, params, device, stream)
    assert L.sdfr_init_hypotheses(q, 16, q, 576, q, 0, q, q, 0, None) == -1 and b"N=0" in err()
    assert L.sdfr_init_hypotheses(q, 16, q, 576, q, 33, q, q, 0, None) == -1 and b"N=33" in err()
    assert L.sdfr_init_hypotheses(q, 7, q, 576, q, 4, q, q, 0, None) == -1 and b"n_params=7" in err()
    assert L.sdfr_init_hypotheses(q, 16, q, 0, q, 4, q, q, 0, None) == -1 and b"C=0" in err()
    for hole in range(5):
        args = [q, 16, q, 576, q, 4, q, q]
        args[(0, 2, 4, 6, 7)[hole]] = None
        assert L.sdfr_init_hypotheses(*args, 0, None) == -2 and b"sdfr_init_hypotheses: NULL" in err()
    # sdfr_select_row(score, score_stride, N, rows, n, out_row, out_index, out_score, device, stream)
    assert L.sdfr_select_row(q, 1, 0, q, 16, q, q, q, 0, None) == -1 and b"N=0" in err()
    assert L.sdfr_select_row(q, 1, 33, q, 16, q, q, q, 0, None) == -1 and b"N=33" in err()
    assert L.sdfr_select_row(q, 0, 4, q, 16, q, q, q, 0, None) == -1 and b"score_stride=0" in err()
    assert L.sdfr_select_row(q, 1, 4, q, -1, q, q, q, 0, None) == -1
    for hole in (0, 3, 5, 6, 7):
        args = [q, 1, 4, q, 16, q, q, q]
        args[hole] = None
        assert L.sdfr_select_row(*args, 0, None) == -2 and b"sdfr_select_row: NULL" in err()


def test_twin_ranking_hand_written_cases():
    nan = np.nan
    # ties: the smaller index first
    idx, prob = twin.topk([0.1, 0.4, 0.4, 0.05, 0.4], 4)
    assert idx.tolist() == [1, 2, 4, 0] and prob.tolist() == [np.float32(0.4)] * 3 + [np.float32(0.1)]
    # one NaN: below every number, taken only when nothing else is left
    idx, prob = twin.topk([nan, 0.0, 0.3, 0.2], 4)
    assert idx.tolist() == [2, 3, 1, 0] and np.isnan(prob[3])
    assert twin.topk([nan, 0.0, 0.3, 0.2], 1)[0].tolist() == [2]
    # all equal: index order; -0 is +0
    assert twin.topk([0.25] * 6, 6)[0].tolist() == [0, 1, 2, 3, 4, 5]
    assert twin.topk([0.0, -0.0, 0.0], 3)[0].tolist() == [0, 1, 2]
    # the maximum at the last index
    assert twin.topk([0.1, 0.2, 0.3, 0.9], 2)[0].tolist() == [3, 2]
    # three non-zero entries, five asked for: the zeros fill in index order
    assert twin.topk([0, 0.2, 0, 0, 0.5, 0, 0.3, 0], 5)[0].tolist() == [4, 6, 1, 0, 2]
    # negative numbers and infinities order as numbers
    assert twin.topk([-1.0, -np.inf, 2.0, np.inf, -0.5], 5)[0].tolist() == [3, 2, 4, 0, 1]


def test_twin_selection_hand_written_cases():
    rows = np.arange(12, dtype=np.float32).reshape(4, 3)
    j, s, r = twin.select_row([0.2, 0.7, 0.7, 0.1], rows)
    assert (j, s, r.tolist()) == (1, np.float32(0.7), [3.0, 4.0, 5.0])
    assert twin.select_row([np.nan, np.nan, 0.0, 0.0], rows)[0] == 2        # NaNs in front
    assert twin.select_row([np.nan] * 4, rows)[0] == 0                      # all NaN
    assert twin.select_row([0.0] * 4, rows)[0] == 0                         # no iteration: all zero
    assert twin.select_row([0.3], rows[:1])[0] == 0


def _round_f32(x: Fraction) -> np.float32:
    """the float32 nearest to a rational, ties to even, by exact comparison"""
    c = np.float32(float(x))
    cands = sorted({c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))}, key=float)
    best = min(cands, key=lambda f: (abs(Fraction(float(f)) - x), int(np.float32(f).view(np.int32)) & 1))
    return np.float32(best)


def test_twin_product_is_the_exactly_rounded_fused_form():
    rng = np.random.default_rng(3)
    for _ in range(2000):
        a, b, c = (np.float32(v) for v in rng.normal(size=3) * 10.0 ** rng.integers(-3, 4, size=3))
        want = _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))
        assert twin._fma(a, b, c).view(np.int32) == want.view(np.int32)
    # a double rounding trap: a * b = 1 + 2^-11 + 2^-24 is a float32 tie, c lifts the sum just above it, and plain
    # float64 arithmetic loses c and rounds the tie to even, downwards
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -70)
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    assert twin._fma(a, b, c) == _round_f32(exact) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert np.float32(float(a) * float(b) + float(c)) == np.float32(1 + 2.0 ** -11)
    # identities of the product: unit (x) q = q, q (x) conj(q) = |q|^2 (0, 0, 0, 1), and the float64 product to rounding
    q = rng.normal(size=4).astype(np.float32)
    one = np.array([0, 0, 0, 1], dtype=np.float32)
    assert np.array_equal(twin.quat_mul_world(one, q), q)
    for _ in range(50):
        a, b = rng.normal(size=(2, 4)).astype(np.float32)
        ax, ay, az, aw = a.astype(np.float64)
        bx, by, bz, bw = b.astype(np.float64)
        ref = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])
        # four products of magnitude <= |a| |b|, three roundings of partial sums: 4 half-ulps of that magnitude at most
        bound = 4 * 2.0 ** -24 * np.linalg.norm(a.astype(np.float64)) * np.linalg.norm(b.astype(np.float64))
        assert np.max(np.abs(twin.quat_mul_world(a, b).astype(np.float64) - ref)) <= bound


def test_twin_rows_keep_everything_but_the_orientation():
    rng = np.random.default_rng(5)
    one = rng.normal(size=16).astype(np.float32)
    grid = rng.normal(size=(10, 4)).astype(np.float32)
    cam = np.array([0.1, -0.3, 0.2, 0.9], dtype=np.float32)
    rows = twin.init_hypotheses(one, grid, [3, -4, 12, 9], cam)
    assert rows.shape == (4, 16)
    assert np.array_equal(rows[:, :3], np.repeat(one[None, :3], 4, 0)) and np.array_equal(rows[:, 7:], np.repeat(one[None, 7:], 4, 0))
    assert np.array_equal(rows[1, 3:7], twin.quat_mul_world(cam, grid[0]))      # clamped from below
    assert np.array_equal(rows[2, 3:7], twin.quat_mul_world(cam, grid[9]))      # ... and from above
    assert np.array_equal(rows[2], rows[3])
