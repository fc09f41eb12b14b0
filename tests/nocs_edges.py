"""numpy builders of the NOCS fit's edge cases (tests/test_nocs_edges_cpu.py, tests/test_nocs_edges_gpu.py,
tools/make_nocs_edge_seeds.py): flat, mirrored, symmetric and axis-aligned sets, extreme scales, NaN inputs, a final fit
without variance, a sweep over the point counts around the 128-point chunk and the 256-lane block, and exactly planar and
collinear sources.  Everything is a function of fixed seeds; the expected result of a case is tests/nocs_twin.py's.

A case is a dict with source, target (N,3), draws (100,5), ``family`` and, for the directed ones, what it was built
for: ``status`` / ``iterations_run`` / ``branch``.

Rows that sample the same five points in another order are the same hypothesis up to rounding, so rounding decides
which of them wins: always for 5 points (every row), nearly always for 6 (six distinct rows exist).  The runner-up
margin is therefore taken between DISTINCT point sets, and ``same_hypothesis`` is what a test compares a winner by.
"""
import numpy as np

import nocs_twin as tw

REL = 1e-6
SEEDS_FILE = "nocs_edge_seeds.json"


# ---- pieces ----------------------------------------------------------------------------------------------------------
def rotation(rng):
    """a rotation matrix from a uniformly drawn unit quaternion"""
    x, y, z, w = (lambda q: q / np.linalg.norm(q))(rng.standard_normal(4))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def similarity(rng, scale):
    return scale, rotation(rng), rng.uniform(-1, 1, 3) + np.array([0, 0, 2.0])


def shape(rng, n):
    """tools/make_nocs_goldens.py::shape: a bent, uneven surface in [-0.5, 0.5]^3 plus a few interior points"""
    u, v = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
    w = 0.35 * np.sin(3 * u) * np.cos(2 * v) + 0.1 * rng.uniform(-1, 1, n)
    return np.stack([u, v, w], axis=1)


def sample_rows(n, seed):
    """nocs_twin.sample_indices(n, seed), which walks all 64 attempts of every draw; this walks them until one is free"""
    from metrics_twin import philox4x32_10
    ctr = np.zeros((tw.N_ITER, 5, 64, 4), np.uint32)
    ctr[..., 0] = np.arange(tw.N_ITER, dtype=np.uint32)[:, None, None]
    ctr[..., 1] = np.arange(5, dtype=np.uint32)[None, :, None]
    ctr[..., 2] = np.arange(64, dtype=np.uint32)[None, None, :]
    ctr[..., 3] = tw.NOCS_STREAM
    key = (np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF))
    idx = ((philox4x32_10(ctr, key)[..., 0].astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).tolist()
    out = np.zeros((tw.N_ITER, 5), np.int64)
    for i in range(tw.N_ITER):
        used = []
        for d in range(5):
            used.append(next((v for v in idx[i][d] if v not in used), None))
            if used[-1] is None:
                used[-1] = min(set(range(5)) - set(used[:-1]))
        out[i] = used
    return out


def case(source, target, draws, **kw):
    return dict(source=source, target=target, draws=np.asarray(draws, np.int32), **kw)


def same_hypothesis(c, i, j):
    """rows i and j of the case's draws sample the same set of points"""
    return i == j or (i >= 0 and j >= 0 and sorted(c["draws"][i].tolist()) == sorted(c["draws"][j].tolist()))


def final_covariance(c, o):
    """the covariance of the final fit over the twin's inliers"""
    s = np.asarray(c["source"], np.float64)[o["inlier_idx"]]
    t = np.asarray(c["target"], np.float64)[o["inlier_idx"]]
    return (t - t.mean(0)).T @ (s - s.mean(0)) / len(s)


# ---- the margins of tools/make_nocs_goldens.py, recomputed with the twin ---------------------------------------------
def margins(c, o=None, conditioning=True):
    """the list of margins that the case misses (empty: choices of another fp64 implementation can be compared exactly).
    conditioning=False leaves out the three inequalities on singular values (the directed cases are built to miss
    them)."""
    o = tw.ransac(c["source"], c["target"], c["draws"]) if o is None else o
    bad = []
    if len(c["source"]) < 5 or not o["residuals"]:
        return bad
    src, tgt = np.asarray(c["source"], np.float64), np.asarray(c["target"], np.float64)
    res = np.asarray(o["residuals"])
    if np.any(np.abs(res / o["stop_t"] - 1) < REL):
        bad.append("a residual at stop_t")
    best = {}                                   # the smallest residual of every distinct point set
    for r, row in zip(res, c["draws"]):
        if np.isnan(r):                         # (a NaN point: no residual is ever the smallest)
            continue
        key = tuple(sorted(row.tolist()))
        best[key] = min(r, best.get(key, np.inf))
    order = np.sort(list(best.values()))
    if len(order) > 1 and not (order[1] - order[0] > REL * order[0]):
        bad.append("winner and runner-up too close")
    if o["best_iteration"] >= 0:
        idx = c["draws"][o["best_iteration"]]
        d = tw.point_residuals(tw.umeyama(src[idx], tgt[idx])[3], src, tgt)
        if np.any(np.abs(d / o["pass_t"] - 1) < REL):
            bad.append("a point at pass_t")
        if abs(o["inlier_ratio"] - 0.1) < 1e-9:
            bad.append("ratio at 0.1")
    if conditioning:
        rows = c["draws"][:len(res)]
        cs, ct = src[rows] - src[rows].mean(1, keepdims=True), tgt[rows] - tgt[rows].mean(1, keepdims=True)
        sv = np.linalg.svd(np.swapaxes(ct, 1, 2) @ cs / 5, compute_uv=False)
        if not np.all((sv[:, 2] / sv[:, 0] > 1e-7) & (sv[:, 1] * sv[:, 2] / sv[:, 0] ** 2 > 1e-10)):
            bad.append("hypothesis conditioning")
        if o["status"] == tw.OK:
            sv = np.linalg.svd(final_covariance(c, o), compute_uv=False)
            if not sv[0] / (sv[1] + sv[2]) < 1e3:
                bad.append("final covariance")
    return bad


# ---- directed cases ----------------------------------------------------------------------------------------------------
COUNTS = (5, 6, 40)
# z extent / xy extent of the three thicknesses: sigma3 / sigma1 of the covariance goes with its square and comes out at
# about 1e-7, 1e-12 and 1e-18 for the bent surface of `shape`
THIN = {"": 2e-3, "12": 5e-6, "18": 5e-9}


def flat_cases():
    """nearly flat sets under an exact similarity, as they are and mirrored in z"""
    out = {}
    for n in COUNTS:
        rng = np.random.default_rng(300 + n)
        s, R, t = similarity(rng, 0.4)
        base = shape(rng, n)
        draws = sample_rows(n, 300 + n)
        for tag, thin in THIN.items():
            src = base * [1, 1, thin / 0.9]             # (shape's z extent is about 0.9 of its x / y extent)
            out[f"flat{tag}_{n}"] = case(src, s * src @ R.T + t, draws, family="mirrored", branch="rotation")
            out[f"mirror{tag}_{n}"] = case(src, s * (src * [1, 1, -1]) @ R.T + t, draws, family="mirrored",
                                           branch="reflection")
        # the thin axis first: the smallest singular value does not come out of the Jacobi sweeps in the last column
        src = (base * [1, 1, THIN[""] / 0.9])[:, [2, 0, 1]]
        out[f"flatx_{n}"] = case(src, s * src @ R.T + t, draws, family="mirrored", branch="rotation")
        out[f"mirrorx_{n}"] = case(src, s * (src * [-1, 1, 1]) @ R.T + t, draws, family="mirrored", branch="reflection")
    return out


def symmetric_cases():
    corners = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)])
    sets = {"octahedron": np.concatenate([0.5 * np.eye(3), -0.5 * np.eye(3)]), "cube": corners,
            "slab": corners * [1, 1, 0.5]}
    out = {}
    for i, (name, src) in enumerate(sets.items()):
        rng = np.random.default_rng(320 + i)
        s, R, t = similarity(rng, 0.4)
        out[name] = case(src, s * src @ R.T + t, sample_rows(len(src), 320 + i), family="symmetric",
                         branch="repeated" if name != "slab" else "two equal")
    return out


def aligned_cases():
    """target = source and target = 2 source + t over sets whose scatter matrix is exactly diagonal (dyadic
    coordinates, mirror-symmetric in every axis the centroid does not cancel): no Jacobi rotation is needed"""
    a, b, c = 0.5, 0.25, 0.125
    box = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    sets = {5: np.array([[a, 0, 0], [-a, 0, 0], [0, b, 0], [0, -b, 0], [0, 0, c]]),
            6: np.array([[a, 0, 0], [-a, 0, 0], [0, b, 0], [0, -b, 0], [0, 0, c], [0, 0, -c]]),
            40: np.concatenate([box * [a / 2 ** i, b / 2 ** ((i + 1) % 3), c * (1 + i / 4)] for i in range(5)])}
    out = {}
    for n, src in sets.items():
        draws = sample_rows(n, 340 + n)
        out[f"same_{n}"] = case(src, src.copy(), draws, family="aligned", branch="diagonal")
        out[f"double_{n}"] = case(src, 2 * src + [0.25, -0.5, 2.0], draws, family="aligned", branch="diagonal")
    return out


def noisy(seed, n, scale, noise, dtype=np.float64, offset=None, share=0.0):
    """the sweep's recipe: shape under a similarity, Gaussian noise, a share of gross outliers"""
    rng = np.random.default_rng(seed)
    s, R, t = similarity(rng, scale)
    if offset is not None:
        t = np.asarray(offset, np.float64)
    src = shape(rng, n)
    tgt = s * src @ R.T + t + noise * rng.standard_normal((n, 3))
    bad = rng.permutation(n)[:int(round(share * n))]
    tgt[bad] += rng.uniform(-0.5, 0.5, (len(bad), 3))
    return src.astype(dtype), tgt.astype(dtype)


def scale_cases():
    out = {}
    for name, seed, scale, dtype, offset in (("scale_1e-3", 360, 1e-3, np.float64, None),
                                             ("scale_1e3", 361, 1e3, np.float64, None),
                                             ("far_f32", 362, 0.4, np.float32, [3.0, -4.0, 29.5])):
        src, tgt = noisy(seed, 40, scale, 2e-5 * scale, dtype, offset)
        out[name] = case(src, tgt, sample_rows(40, seed), family="scale")
    return out


def nan_cases():
    out = {}
    n = 40
    # in a point that row 0 samples
    src, tgt = noisy(380, n, 0.4, 2e-4)
    draws = sample_rows(n, 380)
    src[draws[0, 2], 1] = np.nan
    out["nan_row0"] = case(src, tgt, draws, family="nan", status=tw.NAN_INPUT, iterations_run=1)
    # in a point that row 7 is the first to sample
    src, tgt = noisy(381, n, 0.4, 2e-4)
    draws = sample_rows(n, 381)
    only = [i for i in draws[7] if i not in draws[:7]]
    tgt[only[0], 0] = np.nan
    out["nan_row7"] = case(src, tgt, draws, family="nan", status=tw.NAN_INPUT, iterations_run=8)
    # in a point that no row samples: the rows are drawn among the first n - 1 points
    src, tgt = noisy(382, n, 0.4, 2e-4)
    src[n - 1, 2] = np.nan
    out["nan_unsampled"] = case(src, tgt, sample_rows(n - 1, 382), family="nan", status=tw.NONE,
                                iterations_run=100)
    return out


def pose_error_case(n, seed):
    src, tgt = noisy(seed, n, 10 ** np.random.default_rng(seed + 7).uniform(-1, 0.5), 2e-4, share=0.5)
    return case(src, tgt, sample_rows(n, seed), family="pose_error", status=tw.POSE_ERROR, iterations_run=100)


def find_pose_error_seed(n, first=0, tries=400):
    """the first seed whose winner keeps one inlier that is not point 0 (printed by tools/make_nocs_edge_seeds.py)"""
    for seed in range(first, first + tries):
        c = pose_error_case(n, seed)
        o = tw.ransac(c["source"], c["target"], c["draws"])
        if o["status"] == tw.POSE_ERROR and o["iterations_run"] == 100 and not margins(c, o, conditioning=False):
            return seed
    raise SystemExit(f"no pose-error seed for {n} points")


def directed_cases(seeds):
    """seeds: the content of tests/golden/nocs_edge_seeds.json"""
    out = {}
    for part in (flat_cases(), symmetric_cases(), aligned_cases(), scale_cases(), nan_cases()):
        out.update(part)
    for n, seed in seeds["pose_error"].items():
        out[f"pose_error_{n}"] = pose_error_case(int(n), seed)
    return out


# ---- the sweep -------------------------------------------------------------------------------------------------------
SWEEP_N = (5, 6, 31, 127, 128, 129, 255, 256, 257, 1025)
SWEEP_DTYPES = ("float32", "float64")
SWEEP_SHARES = (0.0, 0.2, 0.5)
SWEEP_NOISES = (2e-5, 2e-4)
SWEEP_SLOTS = 40
SWEEP_TRIES = 20


def sweep_slot(i):
    """(N, dtype, outlier share, noise, first seed) of slot i: every (N, dtype) pair twice, shares and noises cycled"""
    pair = i % (len(SWEEP_N) * len(SWEEP_DTYPES))
    return (SWEEP_N[pair // 2], SWEEP_DTYPES[pair % 2], SWEEP_SHARES[i % 3], SWEEP_NOISES[(i // 3) % 2], 1000 + 100 * i)


def sweep_case(i, seed):
    n, dtype, share, noise, _ = sweep_slot(i)
    scale = 10 ** np.random.default_rng(seed + 7).uniform(-1, 0.5)
    src, tgt = noisy(seed, n, scale, noise, np.dtype(dtype).type, share=share)
    return case(src, tgt, sample_rows(n, seed), family="sweep")


def find_sweep_seed(i):
    first = sweep_slot(i)[4]
    for seed in range(first, first + SWEEP_TRIES):
        if not margins(sweep_case(i, seed)):
            return seed
    raise SystemExit(f"sweep slot {i}: no seed of {SWEEP_TRIES} passes the margins")


def sweep_cases(seeds):
    return {f"sweep{i:02d}": sweep_case(i, seed) for i, seed in enumerate(seeds["sweep"])}


# ---- degenerate families: the reference defines no single answer -----------------------------------------------------
DEGENERATE_SEEDS = 16


def degenerate_case(kind, n, noise, seed):
    """sources are 8-bit colours, k / 255 - 0.5 in fp32 arithmetic as the correspondence kernel forms them, with one
    (planar) or two (collinear) channels constant; the target is a similarity of them, with or without noise"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 256, (n, 3))
    fixed = rng.permutation(3)[:1 if kind == "planar" else 2]
    k[:, fixed] = k[0, fixed]
    src = (k.astype(np.float32) / np.float32(255) - np.float32(0.5)).astype(np.float64)
    s, R, t = similarity(rng, 10 ** rng.uniform(-1, 0.5))
    tgt = s * src @ R.T + t + noise * rng.standard_normal((n, 3))
    return case(src, tgt, sample_rows(n, seed), family=f"{kind}_{n}_{'noisy' if noise else 'exact'}")


def degenerate_families():
    """{family: [16 cases]}"""
    out = {}
    for f, (kind, n, noise) in enumerate((k, n, e) for k in ("planar", "collinear") for n in (5, 200)
                                         for e in (0.0, 1e-3)):
        cases = [degenerate_case(kind, n, noise, 5000 + 100 * f + j) for j in range(DEGENERATE_SEEDS)]
        out[cases[0]["family"]] = cases
    return out
