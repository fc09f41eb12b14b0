"""CPU: the decoders and scenes of tests/loop_decoders.py are what tests/test_loop_decoders_gpu.py takes them for -- the
construction, the conditions on every scene (asserted here, never loosened on the GPU), and the committed float32
floors of the first gradient."""
import numpy as np
import pytest
import torch

import oracle
import loop_decoders as D


@pytest.fixture(scope="module")
def measured():
    """name -> scene -> loop_decoders.measures (computed once, read only)"""
    return {name: {which: D.measures(D.scene(name, which)) for which in D.SCENES} for name in D.NAMES}


@pytest.mark.parametrize("name", D.NAMES)
def test_construction(name):
    spec = D.FAMILY[name]
    fc, conv = D.layers(spec)
    st = D.state_dict(spec)
    C, s, R = spec["channels"], spec["s"], spec["volume"]
    assert fc[-1]["out"] == C * s ** 3 and len(fc) == len(spec["hidden"]) + 1
    # channel 0 of the last Linear layer carries the shifted sphere and sees no input
    last = len(fc) - 1
    w = st[f"decoder._fc_layers.{last}.weight"].reshape(C, s ** 3, -1)
    b = st[f"decoder._fc_layers.{last}.bias"].reshape(C, s ** 3)
    assert not w[0].any() and w[1:].any()
    np.testing.assert_allclose(b[0], (D.sphere_on_grid(s) + D.SHIFT).ravel(), rtol=1e-6)
    assert b[0].min() > 1.0                              # (the ReLU leaves it alone)
    # the convolutions pass channel 0 through their centre tap; the last one takes the shift off
    for i in range(len(conv)):
        wt = st[f"decoder._conv_layers.{i}.weight"]
        assert wt[0, 0, 1, 1, 1] == 1.0 and np.count_nonzero(wt[0, 0]) == 1
    assert st[f"decoder._conv_layers.{len(conv) - 1}.bias"][0] == -D.SHIFT
    # ... so a decoder whose other channels are silenced puts out the sphere alone, whatever the latent
    quiet = dict(st)
    for i in range(len(conv)):
        wt = quiet[f"decoder._conv_layers.{i}.weight"].copy()
        wt[0, 1:] = 0.0
        quiet[f"decoder._conv_layers.{i}.weight"] = wt
    from test_decoder_gpu import torch_decoder
    z = torch.tensor(D.scene(name)["z0"][None])
    with torch.no_grad():
        a = torch_decoder(quiet, fc, conv, R, z)[0, 0].numpy()
        b0 = torch_decoder(quiet, fc, conv, R, torch.zeros_like(z))[0, 0].numpy()
    # (its corner voxel is the cropped grid's corner cell: sqrt(3) (1 - 3 / s) - RADIUS, 0.14 at s = 5)
    assert np.array_equal(a, b0) and a.min() < -0.2 and a.max() > 0.1
    assert a[R // 2, R // 2, R // 2] < 0 < a[0, 0, 0]     # inside at the centre, outside at a corner
    # the decoded volumes have both signs, and the plain PyTorch statement agrees with the oracle's decoder
    params = oracle.pack_decoder_params(st, len(fc), len(conv))
    for which in D.SCENES:
        sc = D.scene(name, which)
        for zz in (sc["z0"], sc["z_true"]):
            with torch.no_grad():
                vol = D.decode(name, torch.tensor(zz[None]))[0, 0].numpy()
            assert vol.min() < -0.05 and vol.max() > 0.05
            ref = oracle.decoder_forward(params, D.config(spec), zz[None], dtype=np.float64)[0, 0]
            assert np.abs(vol - ref).max() <= 1e-12 * np.abs(ref).max()
    with torch.no_grad():
        v32 = D.decode(name, torch.tensor(sc["z0"][None], dtype=torch.float32), dtype=torch.float32)
    assert v32.dtype == torch.float32 and np.abs(v32[0, 0].numpy() - vol).max() > 0      # (really another precision)


@pytest.mark.parametrize("name", D.NAMES)
def test_scenes_meet_the_conditions(measured, name):
    for which in D.SCENES:
        m = measured[name][which]
        sc = D.scene(name, which)
        assert sc["obs"].shape == ((2, D.H, D.W) if which == "views" else (1, D.H, D.W))
        # enough hit pixels, in the estimate and in the observation, and enough of them shared
        assert m["hits"].min() >= 300 and m["observed"].min() >= 300, (which, m["hits"], m["observed"])
        assert m["overlap"].min() >= 200, (which, m["overlap"])
        # a clean scene by the G7 goldens' definition: no hit test decided by less than 2e-7, and float32 agrees on
        # every pixel's hit
        assert m["min_margin"].min() >= 2e-7, (which, m["min_margin"])
        assert m["same_mask"].all(), which
        # a live latent: it moves the volume, and the first estimate is not at z = 0 (the ReLU masks matter)
        assert m["latent_moves"] >= 1e-3, (which, m["latent_moves"])
        assert np.abs(sc["z0"]).min() > 0
        # ... and the loss sees it: d loss / d latent is non-zero in at least three quarters of its entries
        gz = m["grads"][8:]
        assert len(gz) == D.FAMILY[name]["latent"] and np.count_nonzero(gz) >= 0.75 * len(gz)
        assert D.meets_conditions(m)
        assert np.all(np.isfinite(m["grads"])) and all(np.abs(m["grads"][sl]).max() > 0 for _, sl in D.GROUPS)
    # every number handed to the GPU is float32-exact
    sc = D.scene(name)
    for k in ("obs", "cam_pos", "cam_quat", "p0", "q0", "z0"):
        assert np.array_equal(sc[k], sc[k].astype(np.float32).astype(np.float64)), k
    assert sc["s0"] == float(np.float32(sc["s0"]))
    # object 0 of the multi-object loop is the first view of the two-view scene
    assert np.array_equal(D.scene(name, "object0")["obs"][0], sc["obs"][0])


@pytest.mark.parametrize("name", D.NAMES)
def test_committed_floors_are_the_recomputed_ones(measured, name):
    committed = D.committed_floors()
    assert sorted(committed) == sorted(D.NAMES)
    for which in D.SCENES:
        now = measured[name][which]["floor"]
        got = np.array(committed[name][which])
        assert got.shape == (4,) and np.all(got > 0)
        assert np.all(got <= 2.0 * now) and np.all(now <= 2.0 * got), (which, got, now)
        # float32 is good for these scenes: the floor never widens the bound beyond 1e-3
        assert np.all(D.bound(name, which) >= 1e-4) and np.all(D.bound(name, which) <= 1e-3)


def test_the_family_reaches_the_edges_it_is_there_for():
    """the shapes against csrc/decoder_fc.hpp's constants, stated in plain numbers (the criterion itself is the
    library's: sdfr_decoder_fc_one_wave, asked on the GPU)"""
    def span(spec, gaps):
        w = [spec["latent"]] + spec["hidden"]
        up = (lambda n: (n + 63) // 64 * 64) if gaps else (lambda n: n)
        off = 0
        for a, b in zip(w[:-1], w[1:]):
            off = up(up(off) + a * b)
            end = off + b
            off = end
        return end if len(w) > 1 else 0
    F = D.FAMILY
    assert span(F["one_layer"], True) == 0 and F["one_layer"]["channels"] * F["one_layer"]["s"] ** 3 == 256 + 176
    assert span(F["edge64"], False) == span(F["edge64"], True) == 6110 and 3 * 1536 < 6110 < 6144
    assert span(F["gap"], False) == 6080 <= 6144 < span(F["gap"], True) == 6176
    assert len(F["deep8"]["hidden"]) + 1 == 8 and F["deep8"]["channels"] * F["deep8"]["s"] ** 3 == 250
    assert max(F["wide"]["hidden"]) > 64 and F["wide"]["volume"] != 64 and F["wide"]["channels"] == 3
    assert 8 + F["latent248"]["latent"] == 256 and 8 + D.OVERSIZE["latent"] == 257
    assert max(max([f["latent"]] + f["hidden"]) for n, f in F.items() if f["narrow"]) == 64
