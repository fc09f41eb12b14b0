"""GPU: the initialisation network under eval() on N point sets per launch (SDFPoseNet.features_batch / forward_batch
over csrc/initnet_eval.hip), the validation numbers (sdfr_pose_metrics, pose_metrics, SDFPoseNetTrainer.validate /
geodesic_distance / fit) and the command line's validation, against the float64 twins (tests/init_train_twin.py under
eval(), tests/init_eval_twin.py) and, bit for bit, against the single-set path.

Bounds (Accuracy; tests/golden/init_eval_floors.json holds the floors, test_init_eval_cpu.py re-derives
them): every case's bound is 10 x its own "fp32 floor" -- how far torch fp32 on the CPU lies from float64 on the case's
inputs; 10 x is the project's margin for a summation order that is not torch's.  The forward is continuous, so nothing is
excluded; the inputs keep the top two logits of a sample 1e-3 apart and |q . q*| <= 0.999 (the twin asserts both)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import init_eval_twin as ev
import init_train_twin as tw
from helpers import ROOT

pytestmark = pytest.mark.gpu

MARGIN = 10.0
CLIP_PIN = 2.0 * np.arccos(1.0 - 2.0 ** -23)


@functools.lru_cache(maxsize=None)
def tables():
    return ev.grid_tables()


@functools.lru_cache(maxsize=None)
def reference(case, which):
    """ev.batch of a case: computed once, never modified"""
    return ev.batch(case, which, tables()[case[0]])


@functools.lru_cache(maxsize=None)
def network(name, seed=0):
    from sdfest_amd import SDFPoseNet
    from sdfest_amd.init_train import check_config
    cfg = tw.CONFIGS[name]
    checked = check_config(tw.train_config(cfg))
    return SDFPoseNet(checked["backbone"], checked["head"], cfg["latent_size"], tw.random_state(cfg, seed))


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=torch.int64 if np.asarray(a).dtype == np.int64 else dtype, device="cuda")


def dev_targets(t):
    return {k: dev(v) for k, v in t.items()}


def random_points(name, N, M, seed):
    """uncentred sets (what a caller may hand over), in_size wide"""
    d = tw.CONFIGS[name]["backbone"]["in_size"]
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((N, M, d), generator=g) * 0.05 + 0.01).cuda()


def tuple_equal(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


# ---- accuracy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ev.CASES, ids=ev.case_key)
def test_features_rows_tuple_and_validation_means_match_float64_twin(case):
    """Observed on MI355X: see DESIGN.md 3.16 (the share of each bound that is used)."""
    from sdfest_amd.init_train import pose_metrics
    net, floor = network(case[0], case[2]), ev.load_floors()[ev.case_key(case)]
    rel = lambda got, ref: float((got.double().cpu() - ref).abs().max() / ref.abs().max())
    used, record, s64 = {"features": 0.0, "out": 0.0, "tuple": 0.0}, None, []
    for which in (0, 1):
        cfg, _, x, t, feat, out = reference(case, which)
        xs = dev(x)
        used["features"] = max(used["features"], rel(net.features_batch(xs), feat))
        used["out"] = max(used["out"], rel(net.rows_batch(xs), out))
        got = net.forward_batch(xs)
        assert [tuple(v.shape) for v in got] == [tuple(v.shape) for v in tw.split(out, cfg)]
        for a, b in zip(got, tw.split(out, cfg)):
            used["tuple"] = max(used["tuple"], rel(a, b))
        record = pose_metrics(net, xs, dev_targets(t), record)
        s64.append(ev.sums(out, cfg, t, tables()[case[0]]))
    sums = record.tolist()
    assert sums[4] == sum(case[3])
    m64 = ev.means(s64, case[3])
    for i, k in enumerate(ev.SUMS):
        if k in floor:
            used[k] = abs(sums[i] / sums[4] - m64[k]) / abs(m64[k])
        else:
            assert sums[i] == 0.0 and m64[k] == 0.0          # no NLL for a quaternion head
    print(ev.case_key(case), {k: f"{v:.2e} = {v / (MARGIN * floor[k]):.3f} of the bound" for k, v in used.items()})
    for k, v in used.items():
        assert v <= MARGIN * floor[k], k


def test_prediction_equal_to_the_target_is_distance_zero_not_nan():
    """the clip of |q . q*|: a target that IS the predicted cell's quaternion (fp32, so its norm is 1 only to rounding)
    gives 0 or at most 2 acos(1 - 2^-23) per sample"""
    from sdfest_amd.init_train import pose_metrics
    case = ev.CASES[0]
    net = network(case[0], case[2])
    cfg, _, x, t, _, _ = reference(case, 0)
    xs = dev(x)
    cells = net.rows_batch(xs)[:, cfg["latent_size"] + 4:].argmax(1)
    target = dict(dev_targets(t), quaternion=net.grid_quats()[cells])
    sums = pose_metrics(net, xs, target).tolist()
    assert np.isfinite(sums[2]) and 0.0 <= sums[2] <= sums[4] * CLIP_PIN


# ---- exactness ---------------------------------------------------------------------------------------------------------
EXACT = [("P16", 37), ("P16", 130), ("B16", 65), ("Q16", 1), ("Q16", 64), ("R32", 130), ("R16", 37), ("R16", 65),
         ("mug", 130)]


@pytest.mark.parametrize("name, M", EXACT, ids=[f"{n}-M{m}" for n, m in EXACT])
def test_batch_rows_are_the_single_set_paths_bits(name, M):
    """row n of forward_batch = net(points[n][None]); a set alone, in a batch of 3 and at a larger capacity (the rows
    past counts[n] NaN); a permutation of a set's points; two runs"""
    net = network(name)
    x = random_points(name, 3, M, 7 + M)
    with torch.no_grad():
        batch = net.forward_batch(x)
        feats = net.features_batch(x)
        called = net(x)                                        # N = 3 through __call__: raises on the parent
        assert tuple_equal(batch, called)
        for n in range(3):
            single = net(x[n][None])
            assert tuple_equal([v[n:n + 1] for v in batch], single), n
            assert torch.equal(feats[n], net.features(x[n]))
            assert tuple_equal([v[n:n + 1] for v in batch], net.forward_batch(x[n:n + 1])), n      # N = 1
        wide = torch.full((3, M + 70, x.shape[2]), float("nan"), device="cuda")
        wide[:, :M] = x
        assert tuple_equal(batch, net.forward_batch(wide, counts=[M, M, M]))
        perm = x.clone()
        perm[1] = x[1][torch.randperm(M, generator=torch.Generator().manual_seed(3)).cuda()]
        assert torch.equal(feats, net.features_batch(perm))
        assert tuple_equal(batch, net.forward_batch(x)) and torch.equal(net.rows_batch(x), net.rows_batch(x))


@pytest.mark.parametrize("name", ["P16", "R32", "Q16", "mug"])
def test_ragged_sets_and_an_empty_one(name):
    """counts = [37, 1, 130] at capacity 130, and a set without points among others: every row is the single-set
    path's on the set's own points, the empty set's feature is zero"""
    net = network(name)
    x = random_points(name, 4, 130, 21)
    counts = [37, 0, 130, 1]
    filled = x.clone()
    for n, c in enumerate(counts):
        filled[n, c:] = float("nan")
    with torch.no_grad():
        feats = net.features_batch(filled, counts=torch.tensor(counts))
        rows = net.rows_batch(filled, counts=counts)
        assert torch.equal(feats[1], torch.zeros_like(feats[1])) and torch.isfinite(rows).all()
        for n in (0, 2, 3):
            assert torch.equal(feats[n], net.features(x[n, :counts[n]])), n
        three = net.features_batch(filled[[0, 3, 2]], counts=[37, 1, 130])
        assert torch.equal(three, feats[[0, 3, 2]])


def test_validation_record_same_bits_and_accumulates():
    from sdfest_amd.init_train import pose_metrics
    case = ev.CASES[0]
    net = network(case[0], case[2])
    runs = []
    for _ in range(2):
        record = None
        for which in (0, 1):
            _, _, x, t, _, _ = reference(case, which)
            record = pose_metrics(net, dev(x), dev_targets(t), record)
        runs.append(record)
    assert torch.equal(runs[0], runs[1]) and runs[0].dtype == torch.float64 and runs[0][4] == 4
    _, _, x, t, _, _ = reference(case, 0)
    alone = pose_metrics(net, dev(x), dev_targets(t))
    assert alone[4] == 3 and (alone[:4] < runs[0][:4]).all()
    # without class indices: the same numbers and no NLL
    t3 = {k: v for k, v in dev_targets(t).items() if k != "orientation"}
    bare = pose_metrics(net, dev(x), t3)
    assert torch.equal(bare[:3], alone[:3]) and bare[3] == 0


# ---- the trainer -------------------------------------------------------------------------------------------------------
def eval_batches(case):
    return [(dev(reference(case, w)[2]), dev_targets(reference(case, w)[3])) for w in (0, 1)]


@pytest.mark.parametrize("case", [ev.CASES[0], ev.CASES[3]], ids=ev.case_key)
def test_validate_reads_the_state_and_leaves_it(case):
    from sdfest_amd import SDFPoseNetTrainer
    from sdfest_amd.init_train import pose_metrics, validation_keys
    cfg = tw.CONFIGS[case[0]]
    tr = SDFPoseNetTrainer(tw.train_config(cfg), ev.state(case))
    xt, tt = eval_batches(case)[0]
    tr.step(torch.cat([xt, xt[:1] * 1.5]), {k: torch.cat([v, v[:1]]) for k, v in tt.items()})     # moments, statistics
    before = {k: v.clone() for k, v in tr.state_dict().items()}
    moments = (tr._exp_avg.clone(), tr._exp_avg_sq.clone(), tr._step.clone(), tr.iteration, tr._tracked)
    got = tr.validate(eval_batches(case), "camera")
    after = tr.state_dict()
    assert list(after) == list(before) and all(torch.equal(v, after[k]) for k, v in before.items())
    assert torch.equal(moments[0], tr._exp_avg) and torch.equal(moments[1], tr._exp_avg_sq)
    assert torch.equal(moments[2], tr._step) and moments[3:] == (tr.iteration, tr._tracked) == (1, moments[4])
    keys = validation_keys("camera", bool(cfg["cells"]))
    assert list(got) == keys and len(keys) == (4 if cfg["cells"] else 3)
    assert keys[:3] == ["camera validation mean position error / m", "camera validation mean scale error / m",
                        "camera validation mean geodesic_distance / rad"]
    assert not cfg["cells"] or keys[3] == "camera validation orientation mean NLL"
    net, record = tr.net(), None
    for x, t in eval_batches(case):
        record = pose_metrics(net, x, t, record)
        out = torch.cat([v.reshape(x.shape[0], -1) for v in net.forward_batch(x)], 1)
        raw = net.rows_batch(x)
        assert torch.equal(out[:, :cfg["latent_size"] + 4], raw[:, :cfg["latent_size"] + 4])
    sums = record.tolist()
    assert [got[k] for k in keys] == [sums[i] / sums[4] for i in range(len(keys))]
    assert all(np.isfinite(v) and v > 0 for v in got.values())


@pytest.mark.parametrize("case", ev.TRAIN_CASES, ids=tw.case_key)
def test_training_metric_matches_twin(case):
    """geodesic_distance() after loss_and_grad: the batch mean over the train-mode rows the forward left, within
    10 x the case's floor; computed only when asked, and the call changes nothing"""
    from sdfest_amd import SDFPoseNetTrainer
    cfg, st, x, t, out = ev.train_batch(case, tables()[case[0]])
    ref = float(ev.samples(out, cfg, t, tables()[case[0]])["geodesic"].mean())
    tr = SDFPoseNetTrainer(tw.train_config(cfg), st)
    with pytest.raises(RuntimeError, match="follows"):
        tr.geodesic_distance()
    first = tr.loss_and_grad(dev(x), dev_targets(t))
    got = tr.geodesic_distance()
    assert got.is_cuda and got.dim() == 0
    bound = MARGIN * ev.load_floors()["train-" + tw.case_key(case)]["geodesic"]
    print(f"{tw.case_key(case)}: {float(got):.9g} against {ref:.9g}, {abs(float(got) - ref) / ref / bound:.3f} of the bound")
    assert abs(float(got) - ref) <= bound * ref
    assert torch.equal(got, tr.geodesic_distance())
    again = tr.loss_and_grad(dev(x), dev_targets(t))
    assert all(first[k] == again[k] for k in tw.TERMS) and torch.equal(first["out"], again["out"])
    if cfg["cells"]:        # a discretized head needs the quaternions next to the class indices
        tr.loss_and_grad(dev(x), {k: v for k, v in dev_targets(t).items() if k != "quaternion"})
        with pytest.raises(KeyError, match="quaternion"):
            tr.geodesic_distance()


VIEWS = {"width": 80, "height": 60, "fov_deg": 90, "pointcloud": True, "normalize_pose": True, "render_threshold": 0.004,
         "z_min": 0.2, "z_max": 0.6, "extent_mean": 0.11, "extent_std": 0.01, "mask_noise": False, "norm_noise": False,
         "scale_to_unit_ball": False, "gaussian_noise_probability": 0.0}


@functools.lru_cache(maxsize=None)
def t16_vae():
    import vae_train_twin as vt
    from sdfest_amd import SDFVAE
    state = vt.random_state(vt.T16, 11)
    return vt.T16, state, SDFVAE.from_config(vt.T16, state, sdf_size=vt.T16["sdf_size"])


def small_config(vae_config, **more):
    return tw.train_config(dict(tw.P16, latent_size=vae_config["latent_size"]), batch_size=3, **more)


def generator(seed, batch_size=4):
    from sdfest_amd.generated_views import SDFVAEViewGenerator
    return SDFVAEViewGenerator(dict(VIEWS, orientation_repr="discretized", orientation_grid_resolution=0),
                               t16_vae()[2].decoder, batch_size=batch_size, seed=seed)


def test_validation_set_is_fixed_and_fit_reports_it():
    from sdfest_amd import SDFPoseNetTrainer
    from sdfest_amd.init_train import validation_keys
    vcfg = t16_vae()[0]
    t = SDFPoseNetTrainer(small_config(vcfg), seed=2)
    batches = t.validation_set(generator(9), 8, max_points=64, seed=5)
    assert [b[0].shape[0] for b in batches] == [3, 3, 2] and all(b[0].shape[1] <= 64 for b in batches)
    assert all(sorted(b[1]) == ["latent_shape", "orientation", "position", "quaternion", "scale"] for b in batches)
    again = SDFPoseNetTrainer(small_config(vcfg), seed=77).validation_set(generator(9), 8, max_points=64, seed=5)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1]["quaternion"], b[1]["quaternion"])
               for a, b in zip(batches, again))
    logged = []
    t.fit(generator(6), iterations=4, log_every=1, callback=lambda it, terms: logged.append((it, dict(terms))),
          max_points=64, validation={"camera": batches}, validation_every=2)
    assert [it for it, _ in logged] == [1, 2, 3, 4]
    keys = validation_keys("camera", True)
    for it, terms in logged:
        assert list(terms)[:6] == list(tw.TERMS) + ["metric geodesic distance"]
        assert 0.0 <= terms["metric geodesic distance"] <= np.pi
        assert (list(terms)[6:] == keys) if it % 2 == 0 else (len(terms) == 6), it
        assert all(np.isfinite(v) for v in terms.values())
    # validation iterations are reported even where nothing is logged
    quiet = []
    t.fit(generator(6), iterations=6, log_every=0, callback=lambda it, terms: quiet.append((it, list(terms))),
          max_points=64, validation={"camera": batches}, validation_every=2)
    assert quiet == [(6, keys)]


def test_fit_without_validation_logs_todays_keys_and_bits():
    from sdfest_amd import SDFPoseNetTrainer
    vcfg = t16_vae()[0]
    runs = []
    for extra in ({}, {"validation": None, "validation_every": None}, {"validation": {}, "validation_every": 2}):
        t = SDFPoseNetTrainer(small_config(vcfg), seed=2)
        logged = []
        t.fit(generator(6), iterations=2, log_every=1, callback=lambda it, terms: logged.append((it, dict(terms))),
              max_points=64, **extra)
        assert [it for it, _ in logged] == [1, 2] and all(list(terms) == list(tw.TERMS) for _, terms in logged)
        runs.append((logged, t.state_dict()))
    for logged, state in runs[1:]:
        assert logged == runs[0][0] and all(torch.equal(v, state[k]) for k, v in runs[0][1].items())


def test_command_line_validation(tmp_path):
    import yaml
    vcfg, vstate, _ = t16_vae()
    vae_path, cfg_path, out = str(tmp_path / "vae.pt"), str(tmp_path / "cfg.yaml"), str(tmp_path / "init")
    torch.save({k: torch.tensor(np.asarray(v)) for k, v in vstate.items()}, vae_path)
    config = small_config(vcfg, iterations=4)
    config["vae"] = dict(vcfg, model=vae_path)
    config["datasets"] = {"generated_dataset": {"type": "SDFVAEViewDataset", "probability": 1.0, "config_dict": VIEWS}}
    config["validation_iteration"] = 2
    config["validation_datasets"] = {"camera": {"type": "SDFVAEViewDataset", "config_dict": VIEWS}}
    with open(cfg_path, "w") as fh:
        yaml.safe_dump(config, fh)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_init_network.py"), "--config", cfg_path,
                           "--out", out, "--seed", "4", "--log_every", "0", "--validation_samples", "8"],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr
    with open(out + ".validation.json") as fh:
        history = json.load(fh)
    assert sorted(history) == ["2", "4"]
    for numbers in history.values():
        assert sorted(numbers) == sorted(["camera validation mean position error / m",
                                          "camera validation mean scale error / m",
                                          "camera validation mean geodesic_distance / rad",
                                          "camera validation orientation mean NLL"])
        assert all(np.isfinite(v) for v in numbers.values())
    assert "camera validation mean position error / m" in done.stdout and os.path.exists(out + ".pt")
