"""CPU: the cases of tests/decoder_cases.py are what tests/test_decoder_edges_gpu.py takes them for -- every catalogue
entry and every default seed meets, with its committed sub-draw, the conditions under which a comparison of the decoder
with float64 means something; the committed fp32 floors are what this machine measures; every seed finds a case within
SUB_DRAWS sub-draws; and the layer walk the conditions are measured on is test_decoder_gpu.torch_decoder."""
import pytest
import torch

import decoder_cases as dc
import test_decoder_gpu as D

SEEDS = [f"seed {s}" for s in dc.default_seeds()]


def assert_conditions(c):
    """(a) - (d) of decoder_cases.conditions, one assertion each"""
    what = f"{c.name} (sub-draw {c.sub}): {dc.describe(c.spec)}"
    r = c.report
    print(f"{what}\n    margin {r.margin:.2f}, sides {r.sides:.3f}, floors {r.floor}")
    assert dc.relu_values(c.spec) <= dc.MAX_RELU_VALUES, what
    assert r.margin >= 1.0, f"{what}: a ReLU input within {dc.MARGIN} x torch fp32's deviation of 0"
    assert r.sides >= dc.SIDES, f"{what}: a ReLU'd layer with {r.sides:.3f} of its values on one side"
    for k, v in r.floor.items():
        assert v <= dc.FLOOR, f"{what}: torch fp32 is {v:.2e} from float64 in {k}"
    assert not r.dead, f"{what}: gradients that are identically zero: {r.dead}"
    assert dc.accepted(r)


def assert_floor_is_the_tables(c):
    """the table sets the GPU bounds: it may not lie above what this CPU measures (on one thread) by more than
    HEADROOM -- another CPU's last bits; a table below it only tightens the GPU bounds"""
    entry = dc.load_table()[c.name]
    stored = entry["floor"]
    print(c.name, {k: f"{v:.2e} (table {stored[k]:.2e})" for k, v in c.report.floor.items()})
    assert entry["sub"] == c.sub and sorted(stored) == sorted(c.report.floor)
    for k, v in c.report.floor.items():
        assert stored[k] <= dc.FLOOR and stored[k] <= dc.HEADROOM * v, (c.name, k)


@pytest.mark.parametrize("name", list(dc.CATALOGUE))
def test_edge_meets_the_conditions(name):
    assert 12 <= len(dc.CATALOGUE) <= 18
    c = dc.case(name)
    assert_conditions(c)
    assert_floor_is_the_tables(c)
    assert c.spec["forms"] and c.spec["forms"] <= set(dc.step_names()), name


@pytest.mark.parametrize("name", SEEDS)
def test_seed_finds_a_case_that_meets_the_conditions(name):
    """the search ends within SUB_DRAWS on this machine too, and the case the GPU file runs -- the one the table names
    for the default seeds -- meets the conditions"""
    found = dc.search(name)
    assert found is not None, f"{name}: none of {dc.SUB_DRAWS} sub-draws meets the conditions"
    c = dc.case(name)
    print(f"{name}: the table's sub-draw {c.sub}, this machine's first {found.sub}")
    assert_conditions(c)
    if name in dc.load_table():
        assert_floor_is_the_tables(c)
    assert (name in dc.load_table()) == (int(name.split()[1]) < 16)


def test_the_walk_is_torch_decoder():
    """decoder_cases.walk (which the margins are measured on) computes test_decoder_gpu.torch_decoder's output bit for
    bit, in float64 and in float32, on every catalogue entry and seed"""
    for name in dc.names():
        c = dc.spec(name)
        state, z, _, _ = dc.inputs(name, 0)
        for dtype in (torch.float64, torch.float32):
            zt = torch.tensor(z).to(dtype)
            with torch.no_grad():
                a = dc.walk(c, state, zt, dtype)[0]
                b = D.torch_decoder(state, c["fc"], c["conv"], c["volume"], zt, dtype=dtype)
            assert torch.equal(a, b), (name, dtype)


def test_thresholds_sit_on_both_sides():
    """the pairs of the catalogue straddle the planner's thresholds as their comments say (decoder_plan.hpp, tuning.hpp)"""
    C = dc.CATALOGUE
    n = lambda name: C[name]["N"]
    assert (n("fused_all_n16"), n("fused_all_n17")) == (16, 17)                  # SDFR_SPLITK_MAX_LATENTS
    assert (n("fc65_n31"), n("fc65_n32")) == (31, 32)                            # 4 * kFcSamples
    assert (n("fine32_n7"), n("fine32_n8_folded")) == (7, 8)                     # SDFR_DIRECT_MIN_LATENTS_FEW
    assert 30 * 8 == 240 and 30 * 7 < 240                                        # ... on a layer of 30 tiles
    assert 64 * 2 == 128 and 63 * 2 < 128                                        # N x column tiles (17 channels)
    assert 30 * 30 * 10 * 8 >= 65536 > 30 * 30 * 10 * 7                          # z-grouped (zg = 3)
    for name in ("fused_all_n16", "fused_all_n17", "fc65_n31", "fc65_n32", "fine32_n7", "fine32_n8_folded",
                 "fine32_n8_unfolded", "resident_17ch_n63", "resident_17ch_n64"):
        assert name in C
    # one-wave Linear stack: every input <= 64 and the span of the leading layers' parameters, 64-float alignment gaps
    # included, <= 6144 floats (decoder_fc.hpp, fc_one_wave_ok)
    assert dc.fc_wave_span(C["fc_span_fits"]) == 6110 and dc.fc_wave_span(C["fc_span_gaps"]) == 6176
    raw = lambda c: sum(o * i + o for i, o in zip([c["latent"]] + [l["out"] for l in c["fc"]], [l["out"] for l in c["fc"][:-1]]))
    assert raw(C["fc_span_gaps"]) <= 6144
    assert C["fc65_n31"]["latent"] == 65 and C["fc_span_fits"]["latent"] == 64
    kernels = {l["kernel_size"] for c in C.values() for l in c["conv"]}
    channels = {l[k] for c in C.values() for l in c["conv"] for k in ("in_channels", "out_channels")}
    assert {1, 3, 5} <= kernels and {1, 5, 17} <= channels
    assert any(c["conv"][-1]["relu"] for c in C.values()) and any(c["tsdf"] is not False for c in C.values())
    assert {len(c["fc"]) for c in C.values()} >= {1, 2, 3}


def test_draw_stays_within_its_space():
    for name in SEEDS:
        c = dc.spec(name)
        assert dc.relu_values(c) <= dc.MAX_RELU_VALUES, name
        for l in c["conv"]:
            k3 = l["kernel_size"] ** 3
            assert l["in_channels"] * k3 <= 963 and l["out_channels"] * k3 <= 963, name   # the LDS weight tile
        assert c["conv"][-1]["out_channels"] == 1
        assert all(a["out_channels"] == b["in_channels"] for a, b in zip(c["conv"], c["conv"][1:]))
