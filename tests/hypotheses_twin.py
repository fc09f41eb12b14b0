"""numpy statements of the three rules behind ``sdfr_orientation_topk``, ``sdfr_init_hypotheses`` and ``sdfr_select_row``
(include/sdfr.h), written without looking at how the kernels organise their rounds:

  ranking   ``np.argsort(kind="stable")`` of the negated key, the key being the value with NaN -> -inf: descending
            values, equal values by ascending index (-0 == +0, as numpy compares), a NaN below every finite number
  selection the first entry of that ranking
  product   cam_quat (x) cell quaternion in float32 with the kernel's roundings: per component
            ``fma(+-a1 b, fma(a3 b, +-(a0 b))) +- (a2 b)`` -- two fused steps and two plain products.  ``fma`` is exact
            here: the product of two float32 is exact in float64, and the one float64 sum is rounded to odd before it
            is rounded to float32, which gives the correctly rounded float32 result (53 >= 2 * 24 + 2 bits)."""
import numpy as np

MAX_HYPOTHESES = 32


def rank(values: np.ndarray) -> np.ndarray:
    """all indices of `values`, best first"""
    v = np.asarray(values, dtype=np.float32)
    key = np.where(np.isnan(v), np.float32(-np.inf), v)
    return np.argsort(-key, kind="stable")


def topk(posterior: np.ndarray, n: int):
    """(index (n,) int32, prob (n,) float32: the entries themselves, NaN payloads included)"""
    p = np.asarray(posterior, dtype=np.float32)
    idx = rank(p)[:n].astype(np.int32)
    return idx, p[idx]


def select_row(score: np.ndarray, rows: np.ndarray):
    """(winner, its score, its row)"""
    j = int(rank(score)[0])
    return j, np.asarray(score, dtype=np.float32)[j], np.asarray(rows)[j]


def _fma(a, b, c) -> np.float32:
    """round_to_float32(a * b + c) with ONE rounding, for float32 a, b, c"""
    p = float(a) * float(b)                    # exact: 24 + 24 bits
    c = float(c)
    s = p + c
    if not np.isfinite(s):
        return np.float32(s)
    bb = s - p                                 # TwoSum: s + err == p + c exactly
    err = (p - (s - bb)) + (c - bb)
    if err != 0.0 and (np.float64(s).view(np.int64) & 1) == 0:
        # round to odd: of the two float64 neighbours of the exact sum, take the one with the odd last bit
        s = float(np.nextafter(s, np.inf if err > 0 else -np.inf))
    return np.float32(s)


def quat_mul_world(a, b) -> np.ndarray:
    """a (x) b, scalar last, float32, in ``quat_mul_world``'s (csrc/initnet.hip) order of operations"""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    f32 = np.float32
    return np.array([
        f32(_fma(a[1], b[2], _fma(a[3], b[0], f32(a[0] * b[3]))) - f32(a[2] * b[1])),
        f32(_fma(a[1], b[3], _fma(a[3], b[1], -f32(a[0] * b[2]))) + f32(a[2] * b[0])),
        f32(_fma(-a[1], b[0], _fma(a[3], b[2], f32(a[0] * b[1]))) + f32(a[2] * b[3])),
        f32(_fma(-a[1], b[1], _fma(a[3], b[3], -f32(a[0] * b[0]))) - f32(a[2] * b[2])),
    ], dtype=np.float32)


def init_hypotheses(params_one, grid_quats, index, cam_quat) -> np.ndarray:
    """(N, n) rows: params_one with orientation = cam_quat (x) grid_quats[clamp(index[j])]"""
    params_one = np.asarray(params_one, dtype=np.float32)
    grid_quats = np.asarray(grid_quats, dtype=np.float32)
    rows = np.repeat(params_one[None], len(index), axis=0)
    for j, i in enumerate(index):
        rows[j, 3:7] = quat_mul_world(cam_quat, grid_quats[min(max(int(i), 0), len(grid_quats) - 1)])
    return rows
