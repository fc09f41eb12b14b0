"""GPU: the point cloud term of the VAE trainer (pc_weight; csrc/vae_train.hip: sdfr_vae_trainer_pc_term and
sdfr_vae_trainer_pc_orientations; sdfest_amd.SDFVAETrainer) against its float64 twin (tests/vae_pc_twin.py) and the
reference's golden (tests/golden/vae_train_pc.npz).

The kernel alone, through ctypes, on depth images handed to both sides (the float32 rounding of the float64 oracle's
renders): D = 8 (odd camera, off-centre principal point, fx != fy, one empty image, one image rendered at another pose),
D = 16 with the masked clamp live, D = 64 with the reference's camera.  Then the trainer on the mug config: the seven loss
numbers and every parameter gradient in both phases, determinism, independence of the batch, the orientation draw, the
pc_weight = 0 path, and the command line.

Bounds: those of tests/test_vae_train_gpu.py -- loss numbers 1e-5 relative + 1e-5 absolute, every gradient element 1e-4 of
its tensor's maximum; g_recon likewise 1e-4 of the maximum of the term's gradient.  The twin asserts for every input that
no lifted point lies within 1e-3 of the volume's boundary (in canonical coordinates), so nothing is excluded."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import encoder_twin as et
import oracle
import vae_pc_twin as pt
import vae_train_twin as tw
from helpers import GOLDEN, ROOT
from test_vae_train_cpu import create
from test_vae_train_gpu import PHASES, SEED, close

pytestmark = pytest.mark.gpu

PC_WEIGHT = 0.7        # the kernel tests'; the trainer tests use the configs' 1.0
# W, H, fx, fy, cx, cy (pixel centre 0.5)
KERNEL_CASES = {
    # a 33 x 25 camera, off-centre, fx != fy; sample 0 at a pose and scale of its own, sample 1 an empty image, sample
    # 2's image rendered from (0.7, -0.55, -4.3) but sampled at (0, 0, -5): 71 of its 90 points miss the volume, and the
    # nearest of all lies 1.9e-3 from its boundary (poses chosen on the CPU with the oracle; the twin asserts > 1e-3)
    "d8": dict(config=tw.T8, N=3, camera=(33, 25, 40.0, 35.0, 15.2, 13.9), post=0, key=21,
               position=[(0.1, -0.05, -4.6), pt.POSITION, pt.POSITION], scale=[0.9, 1.0, 1.0],
               render_position=[(0.1, -0.05, -4.6), None, (0.7, -0.55, -4.3)]),
    # the masked clamp (T16: tsdf 0.1) in the post phase
    "d16": dict(config=tw.T16, N=2, camera=(64, 48, 70.0, 70.0, 32.0, 24.0), post=1, key=22,
                position=[pt.POSITION] * 2, scale=[1.0, 1.0], render_position=[pt.POSITION] * 2),
    # the reference's own camera and pose at the size it trains at
    "d64": dict(config=None, N=2, camera=pt.CAMERA, post=0, key=23,
                position=[pt.POSITION] * 2, scale=[1.0, 1.0], render_position=[pt.POSITION] * 2),
}
GOLDEN_CAMERA = (160, 120, 80.0, 80.0, 80.0, 60.0)


def oracle_depth(x, position, quat, scale, camera, dtype=np.float64, with_aux=False):
    W, H, fx, fy, cx, cy = camera
    return oracle.render_forward(np.asarray(x, dtype), position, np.asarray(quat, dtype), [1.0 / scale], W, H, cx, cy,
                                 fx, fy, pt.THRESHOLD, dtype=dtype, with_aux=with_aux)


@functools.lru_cache(maxsize=None)
def kernel_inputs(name):
    """x, recon, depth, pose, the g_recon and terms the loss left, and the twin's (loss_pc, gradient, counts): computed
    once on the CPU, shared, never modified"""
    c = KERNEL_CASES[name]
    config = tw.mug_setup()[0] if c["config"] is None else c["config"]
    D, N = config["sdf_size"], c["N"]
    W, H = c["camera"][:2]
    tsdf = float(config["tsdf"] or 0.0) if c["post"] else 0.0
    rng = np.random.default_rng(c["key"])
    raw = tw.blobs_at(D, tuple(range(N)))[:, 0]
    x = np.clip(raw, -tsdf, tsdf) if tsdf else raw.copy()           # prepare_input
    recon = (raw * 1.3 + rng.normal(0.0, 0.02, raw.shape)).astype(np.float32)
    quats = pt.orientations(c["key"], N)
    depth = np.zeros((N, H, W), np.float32)
    for b, at in enumerate(c["render_position"]):
        if at is not None:
            depth[b] = oracle_depth(x[b], at, quats[b], c["scale"][b], c["camera"])[0].astype(np.float32)
    base = rng.normal(0.0, 0.05, recon.shape).astype(np.float32)
    base[rng.random(recon.shape) < 0.05] = -0.0                     # a voxel the loss left at -0: its bits must survive
    intr = c["camera"][2:]
    loss, grad, counts = pt.term_and_gradient(recon, x, depth, quats, intr, PC_WEIGHT, tsdf, c["position"], c["scale"])
    return dict(config=config, D=D, N=N, x=x, recon=recon, quats=quats, depth=depth, base=base, tsdf=tsdf, loss=loss,
                grad=grad, counts=counts, case=c)


def near(mask):
    """mask (N, D, D, D) grown by one voxel along every axis"""
    m = np.pad(mask, ((0, 0), (1, 1), (1, 1), (1, 1)))
    out = np.zeros_like(mask)
    D = mask.shape[1]
    for a in range(3):
        for b in range(3):
            for c in range(3):
                out |= m[:, a:a + D, b:b + D, c:c + D]
    return out


def run_kernel(k, depth=None, weight=PC_WEIGHT):
    from sdfest_amd import _lib
    L = _lib.lib()
    c = k["case"]
    h = create(L, k["config"])
    dev = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")
    t = {n: dev(v) for n, v in (("depth", k["depth"] if depth is None else depth), ("pos", c["position"]),
                                ("quat", k["quats"]), ("scale", c["scale"]), ("recon", k["recon"]), ("x", k["x"]),
                                ("g", k["base"]))}
    terms = torch.arange(6, dtype=torch.float32, device="cuda") + 100.0
    loss = torch.full((1,), -1.0, device="cuda")
    ws = torch.empty(L.sdfr_vae_trainer_pc_term_workspace_bytes(h, k["N"]), dtype=torch.uint8, device="cuda")
    W, H, fx, fy, cx, cy = c["camera"]
    p = lambda n: t[n].data_ptr()
    rc = L.sdfr_vae_trainer_pc_term(h, p("depth"), k["N"], W, H, cx, cy, fx, fy, p("pos"), p("quat"), p("scale"),
                                    p("recon"), p("x"), c["post"], weight, loss.data_ptr(), terms.data_ptr(), p("g"),
                                    ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0, L.sdfr_last_error()
    L.sdfr_vae_trainer_destroy(h)
    return float(loss.item()), terms.cpu().numpy(), t["g"].cpu().numpy()


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_matches_twin(name):
    """loss_pc, the total and g_recon of sdfr_vae_trainer_pc_term on the twin's depth images.
    Observed on MI355X: see DESIGN.md section 3.14."""
    k = kernel_inputs(name)
    inside = [c[0] for c in k["counts"]]
    assert min(i for i, at in zip(inside, k["case"]["render_position"]) if at is not None) > 10, k["counts"]
    loss, terms, g = run_kernel(k)
    print(f"{name}: points inside / outside {k['counts']}; loss_pc {loss:.6g} (twin {k['loss']:.6g}), uses "
          f"{close(loss, k['loss']):.3f} of the 1e-5 + 1e-5 bound")
    close(terms[5], 105.0 + PC_WEIGHT * k["loss"])
    assert np.array_equal(terms[:5], np.arange(5, dtype=np.float32) + 100.0)
    top = np.abs(k["grad"]).max()
    err = np.abs(g.astype(np.float64) - (k["base"].astype(np.float64) + k["grad"])).max() / top
    print(f"{name}: worst g_recon element {err:.2e} of the term's largest gradient")
    assert top > 0 and err <= 1e-4
    # a voxel no point touches keeps its bits (the -0.0 the loss may have left included).  "No point": not a corner of
    # any point's cell nor a neighbour of one -- float32 may file a point that lies on a cell face under the next cell,
    # whose far corners then receive a weight of rounding size
    untouched = ~near(k["grad"] != 0.0)
    assert np.array_equal(g.view(np.uint32)[untouched], k["base"].view(np.uint32)[untouched])
    assert (g.view(np.uint32)[untouched] == 0x80000000).any()
    # the same bits on a second run
    loss2, terms2, g2 = run_kernel(k)
    assert loss2 == loss and np.array_equal(terms2, terms) and np.array_equal(g2.view(np.uint32), g.view(np.uint32))


def test_kernel_d8_empty_image_and_the_sample_that_misses():
    k = kernel_inputs("d8")
    assert k["counts"][1] == (0, 0)
    inside, outside = k["counts"][2]
    assert outside > 3 * max(inside, 1), k["counts"]          # rendered elsewhere: most points fall outside
    assert not k["grad"][1].any()
    _, _, g = run_kernel(k)
    assert np.array_equal(g[1].view(np.uint32), k["base"][1].view(np.uint32))
    # all-zero depth images: loss_pc 0, the total as it was, g_recon untouched
    loss, terms, g = run_kernel(k, depth=np.zeros_like(k["depth"]))
    assert loss == 0.0 and terms[5] == 105.0
    assert np.array_equal(g.view(np.uint32), k["base"].view(np.uint32))


def test_kernel_d16_corners_the_clamp_cuts():
    """post = 1, tsdf = 0.1: a cut corner contributes the clamped value (the twin's loss_pc is matched only then) and
    receives exactly 0"""
    k = kernel_inputs("d16")
    t = k["tsdf"]
    assert t == 0.1
    cut = (np.abs(k["x"]) >= np.float32(t)) & (np.abs(k["recon"]) > np.float32(t))
    # what the term would give these corners without the clamp's mask: points do touch them
    _, free, _ = pt.term_and_gradient(np.where(cut, np.clip(k["recon"], -t, t), k["recon"]), np.zeros_like(k["x"]),
                                      k["depth"], k["quats"], k["case"]["camera"][2:], PC_WEIGHT, 0.0)
    touched = cut & (free != 0.0)
    assert touched.sum() > 50 and not k["grad"][cut].any()
    loss, _, g = run_kernel(k)
    assert np.array_equal(g.view(np.uint32)[cut], k["base"].view(np.uint32)[cut])
    # the clamp changes the sum by far more than the bound: an unclamped read cannot pass
    unclamped, _, _ = pt.term_and_gradient(k["recon"], k["x"], k["depth"], k["quats"], k["case"]["camera"][2:], PC_WEIGHT)
    assert abs(unclamped - k["loss"]) > 1e-2 * k["loss"]
    close(loss, k["loss"])


def test_weight_zero_gives_the_sum_and_no_gradient():
    k = kernel_inputs("d8")
    loss, terms, g = run_kernel(k, weight=0.0)
    close(loss, k["loss"])
    assert terms[5] == 105.0 and np.array_equal(g.view(np.uint32), k["base"].view(np.uint32))


# ---- the trainer ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(GOLDEN, "vae_train_pc.npz"))
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def mug():
    config, state = tw.mug_setup()
    return dict(config, pc_weight=1.0), state


@functools.lru_cache(maxsize=None)
def trainer():
    from sdfest_amd import Camera, SDFVAETrainer
    W, H, fx, fy, cx, cy = GOLDEN_CAMERA
    return SDFVAETrainer(*mug(), pc_camera=Camera(W, H, fx, fy, cx, cy, pixel_center=0.5))


def inputs(N=2):
    return torch.tensor(tw.blobs_at(64, tuple(range(N))), device="cuda")


def run(phase, N=2, **kw):
    out = trainer().loss_and_grad(inputs(N), seed=SEED, iteration=PHASES[phase], **kw)
    return dict(out, grads={k: v.clone() for k, v in out["grads"].items()})


def check_against(out, terms, grads, what):
    worst, where = 0.0, None
    for name, g64 in grads.items():
        g = out["grads"][name].cpu().numpy().astype(np.float64)
        top = np.abs(g64).max()
        err = np.abs(g - g64).max() / top
        if err > worst:
            worst, where = err, name
    used = max(close(out[k], terms[k]) for k in pt.TERMS)
    print(f"{what}: worst gradient error {worst:.2e} of the tensor's maximum ({where}); the seven numbers use {used:.3f} "
          "of the 1e-5 + 1e-5 bound")
    assert worst <= 1e-4, f"{where}: {worst:.2e} of its maximum"


@pytest.mark.parametrize("phase", list(PHASES))
def test_trainer_matches_twin_and_golden(phase):
    """the mug config with pc_weight = 1 at N = 2, the golden's orientations and camera.  (a) the trainer's own render:
    pc_depth against the float32 oracle (check_depth, margins as tests/test_render_gpu.py), then the seven numbers and
    every parameter gradient against the twin on those very images; (b) the golden's images given as pc_depth: against
    the twin and against the reference's golden (every 97th gradient element, max-abs)."""
    from test_render_gpu import check_depth
    g = golden()
    config, state = mug()
    quats = g["orientations"]
    x = tw.blobs_at(64, (0, 1))
    eps = et.normal_eps(SEED, 2, 8)
    out = run(phase, pc_orientations=quats)
    assert torch.equal(out["pc_orientations"].cpu(), torch.tensor(quats))
    depth = out["pc_depth"].cpu().numpy()
    xc = np.clip(x, -0.1, 0.1) if phase == "post" else x
    for b in range(2):
        d_or, _, margin = oracle_depth(xc[b, 0], pt.POSITION, quats[b], pt.SCALE, GOLDEN_CAMERA, np.float32, True)
        check_depth(depth[b], d_or[0], margin[0], f"{phase}/view{b}")
    terms, grads, _ = pt.Twin(config, state).run(x, eps, PHASES[phase], quats, depth, GOLDEN_CAMERA[2:])
    assert terms["pc"] > 1.0
    check_against(out, terms, grads, f"{phase}, own render")
    # (b)
    given = pt.dense(g[f"{phase}_depth_index"], g[f"{phase}_depth_value"], (2, GOLDEN_CAMERA[1], GOLDEN_CAMERA[0]))
    out = run(phase, pc_orientations=quats, pc_depth=torch.tensor(given, device="cuda"))
    assert torch.equal(out["pc_depth"].cpu(), torch.tensor(given))
    ref = dict(zip(pt.TERMS, g[f"{phase}_terms"]))
    used = max(close(out[k], ref[k]) for k in pt.TERMS)
    worst = 0.0
    for name in g["names"].tolist():
        top = g[f"{phase}/{name}/stats"][0]
        flat = out["grads"][name].cpu().numpy().astype(np.float64).reshape(-1)
        worst = max(worst, np.abs(flat[::int(g["every"])] - g[f"{phase}/{name}/samples"]).max() / top,
                    abs(np.abs(flat).max() - top) / top)
    print(f"{phase}, golden: gradient samples within {worst:.2e} of the tensor's maximum; numbers use {used:.3f}")
    assert worst <= 1e-4


def test_trainer_same_bits_rows_independent_and_device_orientations():
    a, b = run("post"), run("post")
    for k in pt.TERMS:
        assert a[k] == b[k], k
    for k in ("recon", "pc_depth", "pc_orientations"):
        assert torch.equal(a[k], b[k]), k
    for k, g in a["grads"].items():
        assert torch.equal(g, b["grads"][k]), k
    # the draw: the twin's, a function of (seed, index) -- and of the iteration when no seed is given
    assert np.array_equal(a["pc_orientations"].cpu().numpy(), pt.orientations(SEED, 2))
    t = trainer()
    g2 = t._batch[2]["g_recon"].clone()
    one = run("post", N=1)
    assert np.array_equal(one["pc_orientations"].cpu().numpy(), pt.orientations(SEED, 1))
    # a row does not depend on the rest of the batch: its image, and its slice of d total / d recon, term included
    assert torch.equal(one["pc_depth"][0], a["pc_depth"][0]) and torch.equal(one["recon"][0], a["recon"][0])
    assert torch.equal(t._batch[1]["g_recon"][0], g2[0])
    keep, t.iteration, t.seed = (t.iteration, t.seed), 7, 3
    try:
        drawn = t.loss_and_grad(inputs(1))["pc_orientations"].cpu().numpy()
    finally:
        t.iteration, t.seed = keep
    assert np.array_equal(drawn, pt.orientations(pt.iteration_seed(3, 7), 1))


def test_weight_zero_is_the_path_without_the_term():
    """pc_weight = 0 against a trainer constructed without the key: the same bits, and none of the term's outputs"""
    from sdfest_amd import SDFVAETrainer
    config, state = tw.mug_setup()
    assert "pc_weight" not in config
    a, b = SDFVAETrainer(config, state), SDFVAETrainer(dict(config, pc_weight=0.0), state)
    x = inputs()
    for phase in PHASES:
        ra = a.loss_and_grad(x, seed=SEED, iteration=PHASES[phase])
        rb = b.loss_and_grad(x, seed=SEED, iteration=PHASES[phase])
        assert sorted(ra) == sorted(rb) and "pc" not in rb and "pc_depth" not in rb
        assert all(ra[k] == rb[k] for k in tw.TERMS)
        assert all(torch.equal(g, rb["grads"][k]) for k, g in ra["grads"].items())
    for _ in range(2):
        assert torch.equal(a.step(x, seed=1), b.step(x, seed=1))
    assert torch.equal(a._params, b._params) and "pc_ws" not in b._batch[2]
    with pytest.raises(ValueError, match="pc_weight"):
        b.loss_and_grad(x, pc_depth=torch.zeros(2, 480, 640))
    # with the term the step moves the parameters elsewhere, and pc_term holds the sum
    c = SDFVAETrainer(dict(config, pc_weight=1.0), state)
    terms = c.step(x, seed=1)
    assert float(c.pc_term.item()) > 1.0 and not torch.equal(c._params, SDFVAETrainer(config, state)._params)
    assert terms.shape == (6,)


def test_term_asks_the_allocator_for_nothing_per_step():
    """after the first step at a batch size the term adds kernels only: a step with pc_weight = 1 makes as many
    allocator calls as one with pc_weight = 0 (the clone of the six numbers and the copy of x), and its buffers stay"""
    from sdfest_amd import SDFVAETrainer
    config, state = tw.mug_setup()
    x = inputs()
    calls = {}
    for w in (0.0, 1.0):
        t = SDFVAETrainer(dict(config, pc_weight=w), state)
        t.step(x, seed=1)
        held = {k: v.data_ptr() for k, v in t._batch[2].items()}
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        for _ in range(3):
            t.step(x, seed=1)
        calls[w] = torch.cuda.memory_stats()["allocation.all.allocated"] - before
        assert held == {k: v.data_ptr() for k, v in t._batch[2].items()}
    assert calls[1.0] == calls[0.0], calls


def test_fit_through_the_command_line(tmp_path):
    """three iterations of tools/train_vae.py on the mug architecture with pc_weight: 1.0 (the reference's camera):
    the term is printed, and the saved pair loads into SDFVAE.from_config"""
    from sdfest_amd import SDFVAE
    import yaml
    config = dict(tw.mug_setup()[0], pc_weight=1.0, batch_size=2, iterations=3, warm_up_iterations=1)
    folder = tmp_path / "volumes"
    folder.mkdir()
    for i, v in enumerate(tw.blobs_at(64, (0, 1))):
        np.save(str(folder / f"{i:05d}.npy"), v[0])
    cfg_path, out = str(tmp_path / "cfg.yaml"), str(tmp_path / "model")
    with open(cfg_path, "w") as fh:
        yaml.safe_dump(dict(config, dataset_path=str(folder)), fh)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_vae.py"), "--config", cfg_path, "--out", out,
                           "--seed", "4", "--log_every", "1"], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr
    lines = [l for l in done.stdout.splitlines() if l.startswith("iteration ")]
    assert len(lines) == 3 and all(", pc " in l for l in lines), done.stdout
    assert all(float(l.split(", pc ")[1].split(",")[0]) > 0.0 for l in lines)
    with open(out + ".yaml") as fh:
        saved = yaml.safe_load(fh)
    assert saved["pc_weight"] == 1.0 and saved["model"] == "./model.pt"
    model = SDFVAE.from_config(saved, torch.load(out + ".pt", map_location="cpu"), sdf_size=saved["sdf_size"])
    with torch.no_grad():
        z = torch.zeros(1, saved["latent_size"], device="cuda")
        assert torch.isfinite(model.decode(z)).all()
