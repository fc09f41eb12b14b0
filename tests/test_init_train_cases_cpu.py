"""CPU: the cases of tests/init_train_cases.py are what the two GPU files take them for -- every hand-written edge and
every default seed's random architecture meets the conditions under which a comparison of the initialisation network's
trainer with its float64 twin means something, every seed finds its case within the sub-draws it has, the edges together
take every path of the trainer's kernels that the list ``PATHS`` names, the committed table of fp32 floors is what this
machine measures, and the twin's parameter layout is the library's on every edge."""
import numpy as np
import pytest

import init_train_cases as ic
import init_train_twin as tw

SEEDS = ic.default_seeds()


def assert_conditions(c):
    """the conditions of init_train_cases.conditions, one assertion each"""
    what = f"{c.name} (seed {c.seed}, offset {c.offset}): {ic.describe(c.cfg, c.N, c.M)}"
    r = c.report
    print(f"{what}\n    branch margin {r.margin:.2e}, fp32 floor {r.floor}, null tensors {r.nulls}")
    widths = c.cfg["backbone"]["mlp_out_sizes"] + c.cfg["head"]["mlp_out_sizes"]
    assert max(widths) <= 300 and c.N * c.M <= 2100 and ic.check_shape(c.cfg, c.N, c.M), what
    grads = c.reference[1]
    shapes = tw.parameter_shapes(c.cfg)
    assert sorted(grads) == sorted(k for k, _ in shapes) and all(grads[k].shape == tuple(s) for k, s in shapes), what
    assert r.margin >= 1e-5, f"{what}: a value within {r.margin:.2e} of a branch"
    assert not r.bad_nulls, f"{what}: null tensors that are no bias of a batch-normalised part: {r.bad_nulls}"
    assert not r.dead, f"{what}: gradients that are identically zero without a BatchNorm: {r.dead}"
    assert not r.zero_terms, f"{what}: loss terms that are zero: {r.zero_terms}"
    assert r.floor["grad"] <= 1e-4, f"{what}: torch fp32 on the CPU is {r.floor['grad']:.2e} from float64"
    assert r.floor["null"] <= 4.2e-5, f"{what}: torch fp32 leaves {r.floor['null']:.2e} in a null tensor"
    for k in r.nulls:
        assert k.endswith(".bias") and ic.part_of(c.cfg, k)["batchnorm"] and tw.null_scale(k, grads) > 0, (what, k)
    assert ic.accepted(r)


def assert_floor_is_the_tables(c):
    """the table sets the GPU bounds: it may not lie above what this CPU measures (on one thread) by more than another
    CPU's last bits; a table BELOW it only tightens the GPU bounds"""
    entry = ic.load_table()[c.name]
    stored = entry["floor"]
    print(c.name, {k: f"{v:.2e} (table {stored[k]:.2e})" for k, v in c.report.floor.items()})
    assert (entry["seed"], entry["offset"]) == (c.seed, c.offset) and sorted(stored) == sorted(c.report.floor)
    assert stored["grad"] <= 1e-4 and stored["null"] <= 4.2e-5
    for k, v in c.report.floor.items():
        assert stored[k] <= 1.5 * v, (c.name, k)


@pytest.mark.parametrize("name", list(ic.EDGES))
def test_edge_meets_the_conditions(name):
    assert 12 <= len(ic.EDGES) <= 16 and sorted(ic.EDGE_DRAWS) == sorted(ic.EDGES)
    c = ic.edge(name)
    assert_conditions(c)
    assert_floor_is_the_tables(c)
    # its draw is one of the sub-draws, with the offset that sub-draw has, and the search ends on this machine too
    cfg, N, M = ic.EDGES[name]
    assert 0 <= c.seed < ic.SUB_DRAWS and c.offset == ic.sub_draw(cfg, 0, c.seed)[1]
    first = ic.search(name, cfg, N, M, 0)
    assert first is not None
    print(f"{name}: the listed draw {ic.EDGE_DRAWS[name]}, this machine's first {(first.seed, first.offset)}")


@pytest.mark.parametrize("seed", SEEDS)
def test_seed_finds_a_case_that_meets_the_conditions(seed):
    """the search over the sub-draws ends on this machine too, and the case the GPU file runs -- the one the table names
    for the default seeds, so that it is the same case wherever the suite runs -- meets the conditions"""
    found = ic.find(seed)
    assert found is not None, f"seed {seed}: none of {ic.SUB_DRAWS} sub-draws meets the conditions"
    assert ic.roomy(found.report)
    c = ic.case(seed)
    assert c is not None and (c.cfg, c.N, c.M) == ic.architecture(seed)
    assert 0 <= c.seed - 100 * (seed + 1) < ic.SUB_DRAWS and c.offset == ic.sub_draw(c.cfg, 0, c.seed % 100)[1]
    print(f"seed {seed}: the table's draw {(c.seed, c.offset)}, this machine's first {(found.seed, found.offset)}")
    assert_conditions(c)
    if f"seed {seed}" in ic.load_table():
        assert_floor_is_the_tables(c)
    assert (f"seed {seed}" in ic.load_table()) == (seed < 16)


def test_edges_take_every_listed_path():
    took = {name: ic.paths(*ic.EDGES[name]) for name in ic.EDGES}
    for path in ic.PATHS:
        by = [name for name, t in took.items() if path in t]
        print(f"{path}: {', '.join(by)}")
        assert by, f"no edge takes the path {path!r}"
    assert len(set(ic.PATHS)) == len(ic.PATHS)


def test_paths_are_read_from_the_shapes():
    """the path detector on the eleven cases of tests/test_init_train_gpu.py: what they take of PATHS is a one-layer and
    a three-layer head and the mug's 512-wide head layer -- nothing else of the list"""
    took = {tw.case_key(c): ic.paths(tw.CONFIGS[c[0]], c[1], c[2]) for c in tw.CASES}
    for key, t in took.items():
        print(key, sorted(t))
    assert took["mug-N4-M64-s26"] == {"three head layers", "head wider than 256"}
    for key, t in took.items():
        name = key.split("-")[0]
        if name in ("Q16", "R16"):
            assert t == {"one head layer"}, key
        elif name != "mug":
            assert t == set(), key
    # the walk of sdfr_pose_trainer_create, link by link: P16 (dense + residual, 16 16 16 40) and R32 (... 16 16 32)
    assert [(l["cin_f"], l["cin_g"], l["res"], l["out_g"]) for l in ic.links(tw.P16)] == [
        (3, 0, 0, True), (16, 16, 1, True), (16, 16, 1, True), (16, 16, 0, False)]
    assert [l["res"] for l in ic.links(tw.R32)] == [0, 1, 2] and [l["res"] for l in ic.links(tw.R16)] == [0, 1, 1]
    # single paths at their thresholds
    plain = lambda widths, in_size=3: ic.net(in_size, widths, False, False, False, [8], False, 2, 0)
    assert "gemm K > 64, partial last chunk" not in ic.paths(plain([64, 8]), 2, 40)
    assert "gemm K > 64, chunk tail K % 4 != 0" not in ic.paths(plain([68, 8]), 2, 40)
    assert {"gemm K > 64, partial last chunk", "gemm K > 64, chunk tail K % 4 != 0"} <= ic.paths(plain([67, 8]), 2, 40)
    assert "gemm tile spans three samples" in ic.paths(plain([8]), 3, 31) and \
        "gemm tile spans three samples" not in ic.paths(plain([8]), 3, 32) | ic.paths(plain([8]), 2, 31)
    assert "wgrad R % 1024 == 1" in ic.paths(plain([8]), 5, 205) and "wgrad R % 1024 == 1" not in ic.paths(plain([8]), 1, 1)
    for M, path in ((29, "set M just below 32"), (32, "set M just below 32"), (33, "set M just above 32"),
                    (36, "set M just above 32")):
        assert path in ic.paths(plain([8]), 2, M), M
    assert not {"set M just below 32", "set M just above 32"} & (ic.paths(plain([8]), 2, 28) | ic.paths(plain([8]), 2, 37))


def test_links_refuse_what_the_library_refuses():
    """``links`` restates the walk of sdfr_pose_trainer_create: the same residual forms, and a ValueError exactly where
    the library returns SDFR_E_INVALID (argument checks only: no HIP call)"""
    from sdfest_amd import _lib
    L = _lib.lib()
    refused = ic.net(6, [3, 8], False, True, True, [8], False, 2, 0)       # in_size = 2 x the first width, dense + residual
    with pytest.raises(ValueError):
        ic.links(refused)
    rc, h = ic.create(L, refused)
    assert rc == -1 and not h.value and b"residual" in L.sdfr_last_error()
    for seed in SEEDS:
        for attempt in range(3):
            cfg, N, M = ic.draw(seed, attempt)
            try:
                ic.links(cfg)
                ok = True
            except ValueError:
                ok = False
            rc, h = ic.create(L, cfg)
            assert (rc == 0) == ok, ic.describe(cfg, N, M)
            if rc == 0:
                assert (L.sdfr_pose_trainer_tape_bytes(h, N, M) > 0) == ic.check_shape(cfg, N, M)
                L.sdfr_pose_trainer_destroy(h)


@pytest.mark.parametrize("name", list(ic.EDGES))
def test_parameter_layout_is_the_librarys(name):
    """``parameter_shapes`` / ``stat_shapes`` / ``n_out`` of the twin against the library's counts, and against the
    Python trainer's where it can express the head; CPU-only, no HIP call"""
    from sdfest_amd import _lib, init_train
    L = _lib.lib()
    cfg, N, M = ic.EDGES[name]
    rc, h = ic.create(L, cfg)
    assert rc == 0
    try:
        shapes = tw.parameter_shapes(cfg)
        assert L.sdfr_pose_trainer_param_count(h) == sum(int(np.prod(s)) for _, s in shapes)
        assert L.sdfr_pose_trainer_stat_count(h) == 2 * sum(c for _, c in tw.stat_shapes(cfg))
        assert L.sdfr_pose_trainer_output_size(h) == tw.n_out(cfg)
        assert L.sdfr_pose_trainer_tape_bytes(h, N, M) > 0 and L.sdfr_pose_trainer_workspace_bytes(h, N, M) > 0
    finally:
        L.sdfr_pose_trainer_destroy(h)
    if not ic.needs_c(cfg):
        checked = init_train.check_config(tw.train_config(cfg))
        assert init_train.parameter_shapes(checked) == [(k, tuple(s)) for k, s in shapes]
        assert init_train.stat_shapes(checked) == tw.stat_shapes(cfg) and init_train.num_cells(checked) == cfg["cells"]


def test_small_sets_are_moved_off_their_centroid():
    """``tw.inputs`` centres every set: one point alone would be the origin, and no weight behind it had a gradient"""
    cfg = ic.EDGES["m1_residual_never_taken"][0]
    x, t = ic.inputs(cfg, 5, 1, 0)
    assert x.shape == (5, 1, 4) and np.abs(x).min() > 0 and np.array_equal(x, x.astype(np.float32).astype(np.float64))
    x5, t5 = ic.inputs(cfg, 5, 5, 0)
    ref, tref = tw.inputs(cfg, 5, 5, 0)
    assert np.array_equal(x5, ref) and all(np.array_equal(t5[k], tref[k]) for k in tref)
