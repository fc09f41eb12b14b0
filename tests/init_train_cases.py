"""The architectures and batch shapes the initialisation network's trainer (sdfest_amd/csrc/initnet_train.hip) is walked
over, for tests/test_init_train_cases_cpu.py (the cases are what they claim to be), tests/test_init_train_edges_gpu.py
(``EDGES``) and tests/test_init_train_fuzz_gpu.py (``case(seed)``).  Everything but ``run_c`` runs on the CPU, in torch,
through the float64 twin tests/init_train_twin.py, which is used as it is: configs in its format, weights from its
``random_state``, point sets and targets from its ``inputs`` (sets of fewer than four points are moved off their
centroid: a centred set of one point is the origin, and nothing behind a zero input has a gradient).

A case is kept only where a comparison against float64 means something (``conditions``): no value lies within 1e-5 of a
branch it decides, torch fp32 on the CPU stays within 1e-4 of each gradient tensor's float64 maximum, the only tensors
with a vanishing gradient are the biases a batch normalisation removes, and every loss term is there.  ``paths`` reads
from the shapes alone which of the kernels' paths (``PATHS``) a case takes.  ``python tests/init_train_cases.py``
rewrites the table of the seeds' draws and of every case's fp32 floors,
tests/golden/init_train_case_floors.json.  Never reads the reference."""
import collections
import contextlib
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import torch

import init_train_twin as tw

MARGIN = 1e-5            # smallest accepted branch_margin
GRAD_FLOOR = 1e-4        # largest accepted fp32 floor of the gradients, of each tensor's float64 maximum
NULL_FLOOR = 4.2e-5      # ... of the null tensors, of their layer's weight gradient (test_init_train_cpu.py's figure)
SUB_DRAWS = 20
# a draw is CHOSEN only with this factor of room under each of the three figures above, and (where the table is written)
# only if it has that room under three instruction paths of the CPU's BLAS: the fp32 twin's last bits are another CPU's
# summation order -- one and the same case measured 2.0e-5 on one machine and 7.8e-5 on another in a null tensor -- and a
# case picked at a threshold on one machine would miss it on the next
HEADROOM = 1.5
CPU_PATHS = ({}, {"MKL_ENABLE_INSTRUCTIONS": "AVX2", "ATEN_CPU_CAPABILITY": "avx2"},
             {"MKL_ENABLE_INSTRUCTIONS": "SSE4_2", "ATEN_CPU_CAPABILITY": "default"})
OFFSETS = (0.0, 2.0, 3.0)
FLOORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_train_case_floors.json")

# the kernels' constants (initnet_train.hip: kT, kSplitRows, kRowBatch x 4 row groups, the 256 threads of a per-column launch)
TILE, SPLIT_ROWS, ROW_GROUPS, ROW_BATCH, BLOCK = 64, 1024, 4, 8, 256
GRID_CELLS = (72, 576, 4608, 36864)       # SO3Grid(r).num_cells(): what the Python trainer can express


def net(in_size, widths, bn, dense, residual, head, head_bn, latent, cells):
    """a config in the twin's format; cells = 0: a quaternion head"""
    cfg = {"backbone": {"in_size": in_size, "mlp_out_sizes": list(widths), "batchnorm": bool(bn), "dense": bool(dense),
                        "residual": bool(residual)},
           "head": {"in_size": widths[-1], "mlp_out_sizes": list(head), "batchnorm": bool(head_bn)},
           "orientation_repr": "discretized" if cells else "quaternion", "cells": cells, "latent_size": latent}
    if cells in GRID_CELLS:
        cfg["orientation_grid_resolution"] = GRID_CELLS.index(cells)
    return cfg


# name -> (config, N, M).  Widths <= 300 and N M <= 2100: well under a second on the GPU, a second or two for the twins.
EDGES = {
    # one layer as wide as the points, residual: Fp = points is a residual source, no data gradient is ever formed, the
    # maximum is taken over points + relu; N = 1 without any BatchNorm; every GEMM has J = 3 and R = 7 rows
    "points_residual_one_layer": (net(3, [3], False, False, True, [5], False, 2, 0), 1, 7),
    # the same link in front of a second layer under BatchNorm: the backward stops at i == 0 with a residual link
    # pending; 5 cells (no SO3 grid has 5: through the C entry points); M = 33 = 32 + 1
    "points_residual_bn_5_cells": (net(3, [3, 17], True, False, True, [20], True, 3, 5), 4, 33),
    # every width just past a tile: K = 65, 70 (a second k-chunk of 1 and of 6: kp = 4, 8), J = 65, 70, 129 (a second and
    # a third column block of one column), weight-gradient records with C and Fw tails, per-sample passes on 65 and 70
    "widths_65_70_129": (net(3, [65, 70, 129], True, False, False, [66], True, 3, 72), 4, 37),
    # dense without residual and without BatchNorm; data gradients with K = 100 and 67 (67 = 64 + 3: kp = 4 with one
    # padded column); three head layers; M = 65 = one tile + 1
    "dense_plain_50_100_67": (net(3, [50, 100, 67], False, True, False, [30, 20, 10], False, 4, 0), 2, 65),
    # 70 input columns (the first GEMM's K, the first weight gradient's Fw); BatchNorm in the backbone only; N = 3 sets
    # of M = 31: the first 64-row tile spans three samples, and 31 = 32 - 1
    "in_70_backbone_bn": (net(70, [16, 40], True, False, False, [24], False, 3, 72), 3, 31),
    # BatchNorm in the head only, at N = 2; M = 2: two of the four row groups own no row; latent 70: the lane loop of
    # the loss runs twice.  (60 set features: with 24, torch fp32 leaves 4e-5 ... 1e-4 of the head's first weight gradient
    # in that layer's bias at every draw)
    "head_bn_n2_m2_latent_70": (net(3, [16, 60], False, False, False, [24], True, 70, 72), 2, 2),
    # R = 1024: one weight-gradient record, full to the last row (the dense + residual + BatchNorm net of the fixed cases)
    "rows_1024": (tw.P16, 4, 256),
    # R = 1025: a second record made from one row
    "rows_1025": (net(3, [16, 16], False, False, True, [24], False, 2, 0), 5, 205),
    # latent 65 and 130 cells: both lane loops of the loss with a tail (C entry points); a head of 300: the per-column
    # kernels get a second block; M = 5
    "latent_65_130_cells_head_300": (net(3, [16, 24], False, False, False, [300], False, 65, 130), 3, 5),
    # M = 1: three of the four row groups own no row and enter the first-maximum merge with -inf / index 0; the residual
    # flag is set and no link is taken (4 != 6 != 9); 4 input columns; latent 1
    "m1_residual_never_taken": (net(4, [6, 9], False, False, True, [7, 8], False, 1, 72), 5, 1),
    # one input column; dense + residual + BatchNorm with a residual link into a dense link (layer 1) and into the last
    # layer (24 = 12 + 12); M = 3
    "in_1_dense_residual_m3": (net(1, [12, 12, 24], True, True, True, [16], True, 2, 72), 4, 3),
    # one layer with the dense flag set: no maximum is concatenated, no data gradient is formed; M = 64 = one tile
    "one_layer_dense_flag": (net(3, [20], True, True, False, [10], True, 3, 72), 4, 64),
    # the residual links of a dense net past one tile: layer 1 adds [F | G] of 70 + 70 (the maximum's broadcast half in the
    # second column block), the last layer is as wide as both halves together (140: the maximum's gradient is routed
    # into 70 per-point and 70 broadcast columns)
    "dense_residual_70_70_140": (net(3, [70, 70, 140], True, True, True, [24, 16], True, 3, 72), 4, 37),
}
# name -> (seed, offset of random_state): the first of SUB_DRAWS sub-draws at which ``conditions`` hold with HEADROOM on
# every one of CPU_PATHS (``python tests/init_train_cases.py`` checks the list when it writes the table)
EDGE_DRAWS = {
    "points_residual_one_layer": (0, 0.0), "points_residual_bn_5_cells": (2, 3.0), "widths_65_70_129": (1, 2.0),
    "dense_plain_50_100_67": (3, 0.0), "in_70_backbone_bn": (0, 0.0), "head_bn_n2_m2_latent_70": (7, 0.0),
    "rows_1024": (5, 3.0), "rows_1025": (0, 0.0), "latent_65_130_cells_head_300": (0, 0.0),
    "m1_residual_never_taken": (0, 0.0), "in_1_dense_residual_m3": (3, 0.0), "one_layer_dense_flag": (1, 2.0),
    "dense_residual_70_70_140": (5, 3.0),
}


# ---- the link forms, as sdfr_pose_trainer_create walks them ------------------------------------------------------------
def links(cfg):
    """[{cin_f, cin_g, cout, res, last, out_g}] per backbone layer; ValueError for what the library refuses by contract"""
    bb = cfg["backbone"]
    out, fw, gw, n = [], bb["in_size"], 0, len(bb["mlp_out_sizes"])
    for i, c in enumerate(bb["mlp_out_sizes"]):
        last = i == n - 1
        out_g = bool(bb["dense"]) and not last
        res = 0
        if bb["residual"] and fw + gw == c * (2 if out_g else 1):
            if fw == c:
                res = 1
            elif last and gw > 0:
                res = 2
            else:
                raise ValueError(f"layer {i}: a residual link mixing per-point and broadcast columns")
        out.append(dict(cin_f=fw, cin_g=gw, cout=c, res=res, last=last, out_g=out_g))
        fw, gw = c, (c if out_g else 0)
    return out


def check_shape(cfg, N, M):
    """initnet_train.hip: check_shape"""
    return N >= 1 and M >= 1 and (not cfg["backbone"]["batchnorm"] or N * M >= 2) and (not cfg["head"]["batchnorm"] or N >= 2)


def needs_c(cfg):
    """the cell count is none an SO3 grid has: only the C entry points express it"""
    return bool(cfg["cells"]) and cfg["cells"] not in GRID_CELLS


PATHS = (
    "gemm K > 64, partial last chunk", "gemm K > 64, chunk tail K % 4 != 0", "gemm J > 64, partial column block",
    "gemm J < 16", "gemm tile spans three samples", "gemm R below one tile",
    "wgrad R % 1024 == 0", "wgrad R % 1024 == 1", "wgrad Fw > 64 with a tail", "wgrad C > 64 with a tail",
    "set C in 65 ... 127", "set M < 4", "set M = 1", "set M = 2", "set M just below 32", "set M just above 32",
    "residual from the points", "one-layer backbone", "one-layer backbone, dense flag", "dense without residual",
    "residual set, never taken", "dense without BatchNorm", "BatchNorm in the backbone only", "BatchNorm in the head only",
    "head wider than 256", "one head layer", "three head layers", "N = 2 under the head's BatchNorm",
    "N = 1 without BatchNorm", "latent > 64", "latent 1", "cells not 72 * 8^r",
    "in_size 1", "in_size 4", "in_size > 64",
)


def paths(cfg, N, M):
    """which of PATHS the trainer takes on `cfg` at (N, M), from the shapes alone"""
    ls, bb, hd = links(cfg), cfg["backbone"], cfg["head"]
    R, took = N * M, set()

    def take(path, cond):
        if cond:
            took.add(path)

    # train_gemm_rows_kernel: the forward of every layer (K = cin_f, J = cout) and the data gradient of every layer
    # but the first (K = cout, J = cin_f)
    gemms = [(l["cin_f"], l["cout"]) for l in ls] + [(l["cout"], l["cin_f"]) for l in ls[1:]]
    for K, J in gemms:
        take("gemm K > 64, partial last chunk", K > TILE and K % TILE)
        take("gemm K > 64, chunk tail K % 4 != 0", K > TILE and K % 4)
        take("gemm J > 64, partial column block", J > TILE and J % TILE)
        take("gemm J < 16", J < 16)
    take("gemm tile spans three samples", N >= 3 and 2 * M < TILE)       # (the forward's per-sample bias: p / M)
    take("gemm R below one tile", R < TILE)
    take("wgrad R % 1024 == 0", R % SPLIT_ROWS == 0)
    take("wgrad R % 1024 == 1", R > SPLIT_ROWS and R % SPLIT_ROWS == 1)
    for l in ls:
        take("wgrad Fw > 64 with a tail", l["cin_f"] > TILE and l["cin_f"] % TILE)
        take("wgrad C > 64 with a tail", l["cout"] > TILE and l["cout"] % TILE)
        take("set C in 65 ... 127", TILE < l["cout"] < 2 * TILE)
    span = ROW_GROUPS * ROW_BATCH
    take("set M < 4", M < ROW_GROUPS)
    take("set M = 1", M == 1)
    take("set M = 2", M == 2)
    take("set M just below 32", span - ROW_GROUPS < M <= span)           # one batch, its last slot partly empty
    take("set M just above 32", span < M <= span + ROW_GROUPS)           # a second batch for some row groups only
    take("residual from the points", ls[0]["res"] == 1)
    take("one-layer backbone", len(ls) == 1)
    take("one-layer backbone, dense flag", len(ls) == 1 and bb["dense"])
    take("dense without residual", bb["dense"] and not bb["residual"] and len(ls) > 1)
    take("residual set, never taken", bb["residual"] and not any(l["res"] for l in ls))
    take("dense without BatchNorm", bb["dense"] and not bb["batchnorm"] and len(ls) > 1)
    take("BatchNorm in the backbone only", bb["batchnorm"] and not hd["batchnorm"])
    take("BatchNorm in the head only", hd["batchnorm"] and not bb["batchnorm"])
    take("head wider than 256", max(hd["mlp_out_sizes"]) > BLOCK)
    take("one head layer", len(hd["mlp_out_sizes"]) == 1)
    take("three head layers", len(hd["mlp_out_sizes"]) == 3)
    take("N = 2 under the head's BatchNorm", N == 2 and hd["batchnorm"])
    take("N = 1 without BatchNorm", N == 1 and not hd["batchnorm"] and not bb["batchnorm"])
    take("latent > 64", cfg["latent_size"] > 64)
    take("latent 1", cfg["latent_size"] == 1)
    take("cells not 72 * 8^r", needs_c(cfg))
    take("in_size 1", bb["in_size"] == 1)
    take("in_size 4", bb["in_size"] == 4)
    take("in_size > 64", bb["in_size"] > TILE)
    assert took <= set(PATHS)
    return took


# ---- the conditions ---------------------------------------------------------------------------------------------------
Report = collections.namedtuple("Report", "margin floor nulls bad_nulls dead zero_terms")
Case = collections.namedtuple("Case", "name cfg N M seed offset state x t report reference")


@contextlib.contextmanager
def one_thread():
    """torch on one CPU thread for the twins: layers this small run far slower when every op is split over a pool of
    threads, and one thread gives the fp32 twin one summation order on every machine"""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(before)


def inputs(cfg, N, M, seed):
    """``tw.inputs``; sets of fewer than four points are moved off their centroid by a per-set shift of the points' size"""
    x, t = tw.inputs(cfg, N, M, seed)
    if M < 4:
        shift = np.random.default_rng(300 + seed).normal(size=(N, 1, x.shape[2])) * 0.03
        x = (x + shift).astype(np.float32).astype(np.float64)
    return x, t


def part_of(cfg, key):
    return cfg["backbone" if key.startswith("_backbone") else "head"]


def fp32_floor(cfg, state, x, t, ref):
    """``tw.fp32_floor`` for a case that is no entry of ``tw.CASES``: torch fp32 on the CPU against the float64 `ref`"""
    t64, g64, o64, s64 = ref
    t32, g32, o32, s32 = tw.Twin(cfg, state, torch.float32).loss_and_grad(x, t)
    worst, _, null = tw.compare(g32, g64, tw.null_tensors(g64))
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    return {"grad": float(worst), "null": float(null), "terms": float(max(abs(t32[k] - t64[k]) / abs(t64[k]) for k in tw.TERMS)),
            "out": rel(o32, o64), "stats": max([rel(s32[k], s64[k]) for k in s64] + [0.0])}


def conditions(cfg, state, x, t):
    """-> (Report, reference): reference = the float64 twin's (terms, grads, out rows, statistics one step on)"""
    with one_thread():
        ref = tw.Twin(cfg, state).loss_and_grad(x, t)
        terms, grads = ref[0], ref[1]
        nulls = tw.null_tensors(grads)
        # a null tensor is a bias of a batch-normalised part, measured against a weight gradient that is there
        bad = [k for k in nulls if not (k.endswith(".bias") and part_of(cfg, k)["batchnorm"] and tw.null_scale(k, grads) > 0)]
        dead = [k for k, g in grads.items() if not part_of(cfg, k)["batchnorm"] and not np.abs(g).max() > 0]
        zero_terms = [k for k in tw.TERMS if not abs(terms[k]) > 0]
        floor = None
        if not bad and not dead and not zero_terms:
            floor = fp32_floor(cfg, state, x, t, ref)
        report = Report(tw.branch_margin(cfg, state, x, t), floor, nulls, bad, dead, zero_terms)
    return report, ref


def accepted(report):
    return (not report.bad_nulls and not report.dead and not report.zero_terms and report.margin >= MARGIN
            and report.floor is not None and report.floor["grad"] <= GRAD_FLOOR and report.floor["null"] <= NULL_FLOOR)


def roomy(report):
    """``accepted`` with HEADROOM to spare: what ``search`` picks by"""
    return (accepted(report) and report.margin >= HEADROOM * MARGIN and report.floor["grad"] <= GRAD_FLOOR / HEADROOM
            and report.floor["null"] <= NULL_FLOOR / HEADROOM)


def setup(name, cfg, N, M, seed, offset):
    state = tw.random_state(cfg, seed, offset)
    x, t = inputs(cfg, N, M, seed)
    report, ref = conditions(cfg, state, x, t)
    return Case(name, cfg, N, M, seed, offset, state, x, t, report, ref)


def sub_draw(cfg, base, sub):
    """(seed, offset) of sub-draw `sub`: a backbone without BatchNorm has no bias to offset"""
    return base + sub, (OFFSETS[sub % 3] if cfg["backbone"]["batchnorm"] else 0.0)


def search(name, cfg, N, M, base):
    """the first of SUB_DRAWS sub-draws of (state and input seed, offset) that ``conditions`` hold for with HEADROOM to
    spare, or None"""
    for sub in range(SUB_DRAWS):
        c = setup(name, cfg, N, M, *sub_draw(cfg, base, sub))
        if roomy(c.report):
            return c
    return None


@functools.lru_cache(maxsize=None)
def edge(name):
    cfg, N, M = EDGES[name]
    return setup(name, cfg, N, M, *EDGE_DRAWS[name])


# ---- the random walk --------------------------------------------------------------------------------------------------
POINT_COUNTS = (1, 2, 3, 5, 31, 33, 64, 100, 257, 700)
MAX_ROWS = 2100


def draw(seed, attempt=0):
    """a seeded (config, N, M); may be one the library refuses (``case`` draws again)"""
    rng = np.random.default_rng([0x1217, seed, attempt])
    pick = lambda values: values[int(rng.integers(len(values)))]
    width = lambda: int(rng.integers(2, 141))
    in_size = pick((3, 3, 3, 1, 4, 6))
    bn, dense, residual, head_bn = (bool(rng.random() < 0.5) for _ in range(4))
    # BatchNorm in the head alone stays with its edge: behind a backbone without BatchNorm the set features are of the
    # points' size (0.05) and the head's first weight gradient with them, so torch fp32 leaves 1e-4 ... 2e-4 of it in that
    # layer's bias (NULL_FLOOR is 4.2e-5), and where every maximum is positive the last backbone bias is a null tensor too
    bn = bn or head_bn
    n = int(rng.integers(1, 5))
    widths = []
    for i in range(n):
        u = rng.random()
        if i == 0:
            widths.append(in_size if u < 0.15 else width())
        elif u < 0.35:
            widths.append(widths[-1])                       # a residual link can be taken
        elif i == n - 1 and u < 0.55:
            widths.append(2 * widths[-1])                   # dense + residual into the last layer
        else:
            widths.append(width())
    head = [int(rng.integers(257, 301)) if rng.random() < 0.125 else width() for _ in range(int(rng.integers(1, 4)))]
    latent, cells = int(rng.integers(1, 71)), pick((0, 72))
    # (the head's BatchNorm over two rows normalises to +-1: what is left of a gradient is eps / variance, which fp32
    # holds to 1e-3 on features of BatchNorm's size, and over three rows torch fp32 still lies 1e-4 ... 2e-4 from float64:
    # the edges have N = 2, on small features)
    N = int(rng.integers(4 if head_bn else 1, 7))
    # what can keep a branch margin and an fp32 floor: without BatchNorm no bias offset moves the ReLU's cut out of the
    # rows, so the pre-activations are held to a few tens of thousands, and to a hundred thousand with it; one point under
    # a dense BatchNorm has weight gradients that are exactly zero (every row is its own maximum); the statistics of a
    # backbone BatchNorm want some sixty rows (at 33 rows fp32 lies 1e-4 ... 1e-3 from float64 in the null tensors)
    elements = lambda M: N * M * sum(widths)
    fits = [M for M in POINT_COUNTS if N * M <= MAX_ROWS and elements(M) <= (100000 if bn else 30000)
            and not (bn and (N * M < 60 or (dense and M == 1)))]
    M = pick(fits or [5])
    return net(in_size, widths, bn, dense, residual, head, head_bn, latent, cells), N, M


def describe(cfg, N, M):
    bb, hd = cfg["backbone"], cfg["head"]
    flags = "".join(f for f, on in (("B", bb["batchnorm"]), ("D", bb["dense"]), ("R", bb["residual"])) if on) or "-"
    return (f"N={N} M={M} in {bb['in_size']} {bb['mlp_out_sizes']} {flags} head {hd['mlp_out_sizes']}"
            f"{' B' if hd['batchnorm'] else ''} latent {cfg['latent_size']} cells {cfg['cells']}")


@functools.lru_cache(maxsize=None)
def architecture(seed):
    """the first draw of `seed` that the library does not refuse by contract"""
    for attempt in range(20):
        cfg, N, M = draw(seed, attempt)
        try:
            links(cfg)
        except ValueError:
            continue
        if check_shape(cfg, N, M):
            return cfg, N, M
    raise AssertionError(f"seed {seed}: no architecture the library takes")


@functools.lru_cache(maxsize=None)
def find(seed):
    """the first sub-draw of `seed`'s architecture that ``search`` picks; None if none of SUB_DRAWS does
    (tests/test_init_train_cases_cpu.py asserts there is one for every default seed)"""
    return search(f"seed {seed}", *architecture(seed), 100 * (seed + 1))


@functools.lru_cache(maxsize=None)
def case(seed):
    """the case of `seed`: the sub-draw the committed table names (the first with room on every one of CPU_PATHS where
    the table was written: the same case on every machine, with the floor that belongs to it), or ``find``'s for a seed
    beyond the table"""
    entry = load_table().get(f"seed {seed}")
    if entry is None:
        return find(seed)
    return setup(f"seed {seed}", *architecture(seed), entry["seed"], entry["offset"])


# ---- the C entry points ---------------------------------------------------------------------------------------------
def create(L, cfg, device=0):
    """(return code, handle) of sdfr_pose_trainer_create; no HIP call"""
    arr = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    bb, hd = cfg["backbone"], cfg["head"]
    a, b = arr(bb["mlp_out_sizes"]), arr(hd["mlp_out_sizes"])
    h = ctypes.c_void_p()
    rc = L.sdfr_pose_trainer_create(bb["in_size"], len(a), a.ctypes.data_as(ctypes.c_void_p), int(bb["batchnorm"]),
                                    int(bb["dense"]), int(bb["residual"]), len(b), b.ctypes.data_as(ctypes.c_void_p),
                                    int(hd["batchnorm"]), cfg["latent_size"], cfg["cells"], device, ctypes.byref(h))
    return rc, h


def run_c(cfg, state, x, t, weights=tw.WEIGHTS):
    """sdfr_pose_trainer_create / forward / loss / backward on cuda:0 with buffers sized by the library's own size
    functions: what ``SDFPoseNetTrainer.loss_and_grad`` returns (terms as floats, "grads", "out"), and "stats": the
    running statistics after a second forward with update_stats = 1.  For the cases whose cell count the Python trainer
    cannot express."""
    from sdfest_amd import _lib
    L = _lib.lib()
    rc, h = create(L, cfg)
    _lib.check(rc, "sdfr_pose_trainer_create")
    try:
        dev = torch.device("cuda", 0)
        f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev).contiguous()
        shapes, stat_shapes = tw.parameter_shapes(cfg), tw.stat_shapes(cfg)
        N, M = x.shape[:2]
        params = f32(np.concatenate([np.ravel(state[k]) for k, _ in shapes]))
        assert params.numel() == L.sdfr_pose_trainer_param_count(h)
        stats = f32(np.concatenate([np.ravel(state[f"{p}.{s}"]) for p, _ in stat_shapes
                                    for s in ("running_mean", "running_var")] + [np.zeros(1)]))
        assert stats.numel() - 1 == L.sdfr_pose_trainer_stat_count(h)
        n_out = L.sdfr_pose_trainer_output_size(h)
        tape_bytes, ws_bytes = L.sdfr_pose_trainer_tape_bytes(h, N, M), L.sdfr_pose_trainer_workspace_bytes(h, N, M)
        assert tape_bytes > 0 and ws_bytes > 0
        tape = torch.empty(tape_bytes, dtype=torch.uint8, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        points, out, g_out = f32(x), torch.empty((N, n_out), device=dev), torch.empty((N, n_out), device=dev)
        grads, terms = torch.zeros_like(params), torch.zeros(5, device=dev)
        latent, position, scale = f32(t["latent_shape"]), f32(t["position"]), f32(t["scale"])
        index = quat = None
        if cfg["cells"]:
            index = torch.tensor(t["orientation"], dtype=torch.int32, device=dev)
        else:
            quat = f32(t["orientation"])
        st = torch.cuda.current_stream(dev).cuda_stream
        p = lambda v: v.data_ptr() if v is not None else None

        def forward(update):
            rc = L.sdfr_pose_trainer_forward(h, p(params), p(stats), p(points), N, M, update, p(out), p(tape), tape.numel(),
                                             p(ws), ws.numel(), st)
            _lib.check(rc, "sdfr_pose_trainer_forward")

        forward(0)
        rc = L.sdfr_pose_trainer_loss(h, p(out), p(latent), p(position), p(scale), p(index), p(quat), N,
                                      *(float(weights[k + "_weight"]) for k in tw.TERMS[:4]), p(terms), p(g_out), p(ws),
                                      ws.numel(), st)
        _lib.check(rc, "sdfr_pose_trainer_loss")
        rc = L.sdfr_pose_trainer_backward(h, p(params), p(points), N, M, p(tape), p(g_out), p(grads), p(ws), ws.numel(), st)
        _lib.check(rc, "sdfr_pose_trainer_backward")
        result = dict(zip(tw.TERMS, terms.tolist()))
        result["out"] = out.clone()
        flat, off, result["grads"] = grads.clone(), 0, {}
        for key, shape in shapes:
            n = int(np.prod(shape))
            result["grads"][key] = flat[off:off + n].view(shape)
            off += n
        forward(1)
        torch.cuda.synchronize(dev)
        off, result["stats"] = 0, {}
        for prefix, c in stat_shapes:
            result["stats"][prefix + ".running_mean"] = stats[off:off + c].clone()
            result["stats"][prefix + ".running_var"] = stats[off + c:off + 2 * c].clone()
            off += 2 * c
        return result
    finally:
        L.sdfr_pose_trainer_destroy(h)


# ---- the floors -------------------------------------------------------------------------------------------------------
def default_seeds():
    return range(int(os.environ.get("SDFR_FUZZ_SEEDS", "16")))


def sub_draw_flags(seeds=range(16)):
    """name -> [``roomy`` of sub-draw 0, 1, ...] for every edge and seed, on the instruction path this process runs on"""
    todo = [(name, *EDGES[name], 0) for name in EDGES] + [(f"seed {s}", *architecture(s), 100 * (s + 1)) for s in seeds]
    return {name: [roomy(setup(name, cfg, N, M, *sub_draw(cfg, base, sub)).report) for sub in range(SUB_DRAWS)]
            for name, cfg, N, M, base in todo}


def compute_table(seeds=range(16)):
    """name -> {seed, offset, floor} of every edge and default seed: the first sub-draw that is ``roomy`` on every one of
    CPU_PATHS (a process each: the BLAS picks its path when it loads), with the floor this process measures"""
    flags = []
    for env in CPU_PATHS:
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--sub-draws"], env=dict(os.environ, **env),
                              capture_output=True, text=True, check=True)
        flags.append(json.loads(done.stdout))
    table = {}
    for name in flags[0]:
        subs = [sub for sub in range(SUB_DRAWS) if all(f[name][sub] for f in flags)]
        assert subs, f"{name}: no sub-draw has room on every path"
        if name in EDGES:
            cfg, N, M = EDGES[name]
            assert EDGE_DRAWS[name] == sub_draw(cfg, 0, subs[0]), (name, "EDGE_DRAWS should hold", sub_draw(cfg, 0, subs[0]))
            c = edge(name)
        else:
            seed = int(name.split()[1])
            cfg, N, M = architecture(seed)
            c = setup(name, cfg, N, M, *sub_draw(cfg, 100 * (seed + 1), subs[0]))
        table[name] = {"seed": c.seed, "offset": c.offset, "floor": c.report.floor}
    return table


@functools.lru_cache(maxsize=None)
def load_table():
    with open(FLOORS) as fh:
        return json.load(fh)


def tabled(c):
    """the case's report with the committed floor in the place of the one this machine measures: what the GPU tests judge
    by, so that the fp32 twin of the machine they run on has no say (the CPU file re-derives the table)"""
    return c.report._replace(floor=floor_of(c))


def floor_of(c):
    """the committed floor of a case; a seed beyond the table's (SDFR_FUZZ_SEEDS above 16) has the one just measured"""
    entry = load_table().get(c.name)
    assert entry is None or (entry["seed"], entry["offset"]) == (c.seed, c.offset), c.name
    return entry["floor"] if entry else c.report.floor


if __name__ == "__main__":
    if sys.argv[1:] == ["--sub-draws"]:
        print(json.dumps(sub_draw_flags()))
        sys.exit(0)
    table = compute_table()
    with open(FLOORS, "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for k, v in table.items():
        print(k, v["seed"], v["offset"], {n: f"{e:.2e}" for n, e in v["floor"].items()})
