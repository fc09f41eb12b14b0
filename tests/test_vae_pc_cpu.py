"""CPU: the point cloud term of the VAE trainer (pc_weight; sdfest/vae/scripts/train.py:230-269): what the config check
accepts, the float64 twin (tests/vae_pc_twin.py) against the reference's golden (tests/golden/vae_train_pc.npz,
tools/make_vae_pc_goldens.py), the twin's orientation draw, and the argument checks of the two new entry points of the C
ABI's group 10 (no HIP call is made)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import encoder_twin as et
import vae_pc_twin as pt
import vae_train_twin as tw
from helpers import GOLDEN
from test_vae_train_cpu import create


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "vae_train_pc.npz"))
    return {k: g[k] for k in g.files}


def mug_config(**extra):
    config, state = tw.mug_setup()
    return dict(config, pc_weight=1.0, **extra), state


def test_config_check_accepts_the_term_at_64_and_rejects_other_sizes():
    from sdfest_amd.train import PC_CAMERA, PC_POSITION, PC_SCALE, PC_THRESHOLD, check_config
    cfg = check_config(mug_config()[0])
    assert cfg["pc_weight"] == 1.0 and cfg["sdf_size"] == 64
    assert check_config(dict(mug_config()[0], pc_weight=0.0))["pc_weight"] == 0.0
    with pytest.raises(NotImplementedError, match="pc_weight.*sdf_size = 64 only.*no technical reason"):
        check_config(dict(tw.T16, pc_weight=1.0))
    with pytest.raises(NotImplementedError, match="pc_weight"):
        check_config(dict(tw.T8, pc_weight=0.5))
    assert check_config(dict(tw.T16, pc_weight=0.0))["sdf_size"] == 16
    # the reference's literals (train.py:155, :255-263)
    assert (PC_POSITION, PC_SCALE, PC_THRESHOLD) == (pt.POSITION, pt.SCALE, pt.THRESHOLD) == ((0.0, 0.0, -5.0), 1.0, 0.01)
    cam = PC_CAMERA
    assert (cam.width, cam.height) + cam.get_pinhole_camera_parameters(0.5)[:4] == pt.CAMERA
    assert cam.get_pinhole_camera_parameters(0.0)[2:4] == (319.5, 239.5)


@pytest.mark.parametrize("phase, iteration", [("warm", 0), ("post", 1001)])
def test_twin_reproduces_reference_golden(golden, phase, iteration):
    """both are float64 torch: only the summation order can differ -- the seven numbers to 1e-9 relative, gradient
    samples and norms to 1e-9 of each tensor's max-abs (the bound vae_train_twin is held to)"""
    config, state = mug_config()
    W, H, fx, fy, cx, cy = golden["camera"]
    shape = (2, int(H), int(W))
    depth = pt.dense(golden[f"{phase}_depth_index"], golden[f"{phase}_depth_value"], shape)
    assert depth.dtype == np.float32 and np.count_nonzero(depth) > 500
    quats = golden["orientations"]
    assert np.array_equal(quats, pt.orientations(int(golden["seed"]), 2))
    twin = pt.Twin(config, state)
    terms, grads, _ = twin.run(tw.blobs_at(64, (0, 1)), et.normal_eps(int(golden["seed"]), 2, 8), iteration, quats, depth,
                               (fx, fy, cx, cy))
    got = np.array([terms[k] for k in pt.TERMS])
    ref = golden[f"{phase}_terms"]
    assert ref[6] > 1.0 and np.all(np.abs(got - ref) <= 1e-9 * np.abs(ref)), (got, ref)
    # the term is in the total, and it moves the gradients: without it the golden of the five-term iteration comes out
    five = np.load(os.path.join(GOLDEN, "vae_train_mug.npz"))
    assert abs(ref[5] - ref[6] - five[f"{phase}_terms"][5]) <= 1e-9 * ref[5]
    assert sorted(grads) == sorted(golden["names"].tolist())
    every, moved = int(golden["every"]), 0
    for name, g in grads.items():
        top, norm = golden[f"{phase}/{name}/stats"]
        flat = g.reshape(-1)
        assert top > 0, name
        assert abs(np.abs(flat).max() - top) <= 1e-9 * top, name
        assert abs(np.sqrt((flat * flat).sum()) - norm) <= 1e-9 * top * np.sqrt(flat.size), name
        assert np.max(np.abs(flat[::every] - golden[f"{phase}/{name}/samples"])) <= 1e-9 * top, name
        moved += abs(norm - five[f"{phase}/{name}/stats"][1]) > 1e-6 * norm
    assert moved == len(grads)


def test_term_gradient_is_the_trilinear_scatter_and_respects_the_clamp():
    """a 4^3 volume and two hand-placed points: the autograd gradient is 2 w v (trilinear weight) per corner, a corner
    the clamp cuts contributes the clamped value and receives exactly 0, a point outside contributes nothing"""
    D, tsdf = 4, 0.1
    rng = np.random.default_rng(3)
    recon = rng.uniform(-0.09, 0.09, (1, D, D, D))
    x = rng.uniform(-0.09, 0.09, (1, D, D, D))
    recon[0, 1, 1, 1], x[0, 1, 1, 1] = 0.5, 0.3          # cut by the clamp
    recon[0, 2, 1, 1], x[0, 2, 1, 1] = 0.1, 0.3          # at equality: clamped to itself, gradient passes
    # identity orientation, position (0, 0, -5): pixel (row 1, col 1) of a 3 x 3 image with cx = cy = 1.5 looks down -z
    depth = np.zeros((1, 3, 3), np.float32)
    depth[0, 1, 1] = 5.0 - 0.05                          # o = (0, 0, 0.05): cell (1, 1, 1), offsets (0.5, 0.5, 0.575)
    depth[0, 0, 0] = 9.0                                 # far outside
    quats = np.array([[0.0, 0.0, 0.0, 1.0]])
    loss, grad, counts = pt.term_and_gradient(recon, x, depth, quats, (100.0, 100.0, 1.5, 1.5), 0.5, tsdf)
    assert counts == [(1, 1)]
    f = np.array([0.5, 0.5, (5.0 - np.float64(depth[0, 1, 1]) + 1) * 1.5 - 1])
    clamped = recon.copy()
    clamped[0, 1, 1, 1] = tsdf
    v, w = 0.0, {}
    for k in range(8):
        i = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
        w[i] = np.prod([f[a] if i[a] else 1 - f[a] for a in range(3)])
        v += w[i] * clamped[0, 1 + i[0], 1 + i[1], 1 + i[2]]
    assert abs(loss - v * v) <= 1e-12
    expect = np.zeros_like(grad)
    for i, wk in w.items():
        expect[0, 1 + i[0], 1 + i[1], 1 + i[2]] = 2 * 0.5 * v * wk
    expect[0, 1, 1, 1] = 0.0
    assert grad[0, 1, 1, 1] == 0.0 and grad[0, 2, 1, 1] != 0.0
    assert np.max(np.abs(grad - expect)) <= 1e-15
    with pytest.raises(AssertionError, match="boundary"):     # the margin check: a point 5e-4 inside the +z face
        depth[0, 1, 1] = 5.0 - 0.9995
        pt.term_and_gradient(recon, x, depth, quats, (100.0, 100.0, 1.5, 1.5), 0.5, tsdf)


def test_orientations_are_unit_and_a_function_of_seed_iteration_and_index():
    a = pt.orientations(pt.iteration_seed(3, 7), 64)
    assert a.dtype == np.float32 and a.shape == (64, 4)
    assert np.max(np.abs(np.linalg.norm(a.astype(np.float64), axis=1) - 1.0)) <= 2e-7
    # the index alone picks a row: the batch size does not matter
    assert np.array_equal(a[:5], pt.orientations(pt.iteration_seed(3, 7), 5))
    assert np.array_equal(a, pt.orientations(pt.iteration_seed(3, 7), 64))
    # another iteration or another seed: another draw; the key is the trainer's own function of the two
    assert not np.array_equal(a, pt.orientations(pt.iteration_seed(3, 8), 64))
    assert not np.array_equal(a, pt.orientations(pt.iteration_seed(4, 7), 64))
    assert len({tuple(r) for r in a.tolist()}) == 64
    from sdfest_amd.train import SDFVAETrainer
    t = SDFVAETrainer.__new__(SDFVAETrainer)     # the method alone: no GPU
    t.seed, t.iteration = 3, 7
    assert t._iteration_seed(None) == pt.iteration_seed(3, 7)
    # uniform on SO(3): w^2 + z^2 = u1 is uniform on [0, 1); 4096 draws, mean within 4 sigma of 1/2
    u1 = np.sum(pt.orientations(11, 4096).astype(np.float64)[:, 2:] ** 2, axis=1)
    assert abs(u1.mean() - 0.5) < 4 * np.sqrt(1 / 12 / 4096) and u1.min() >= 0.0 and u1.max() < 1.0 + 1e-6
    # the noise of the same key is another stream (counter word 3)
    assert pt.PC_STREAM == 0x56415043 != et.NOISE_STREAM


def test_new_entry_points_validate_their_arguments_without_gpu():
    """sdfr_vae_trainer_pc_term and sdfr_vae_trainer_pc_orientations report argument errors before any HIP call, in the
    group's convention: -1 / -2 / -3 with sdfr_last_error naming the function and the argument"""
    from sdfest_amd import _lib
    L = _lib.lib()
    err = lambda: L.sdfr_last_error()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)   # a non-NULL pointer that is never dereferenced
    h = create(L, tw.T16)
    big = 1 << 40
    cam = (33, 25, 15.5, 13.0, 40.0, 35.0)   # W, H, cx, cy, fx, fy
    ok = [h, q, 2, *cam, q, q, q, q, q, 1, 1.0, q, q, q, q, big, None]
    assert L.sdfr_vae_trainer_pc_term(None, *ok[1:]) == -2 and b"sdfr_vae_trainer_pc_term: NULL trainer" in err()
    for n in (0, -1, 70000):
        args = list(ok)
        args[2] = n
        assert L.sdfr_vae_trainer_pc_term(*args) == -1 and b"sdfr_vae_trainer_pc_term: N=%d" % n in err()
    for i, v in ((3, 0), (3, 70000), (4, 0), (4, -3)):
        args = list(ok)
        args[i] = v
        assert L.sdfr_vae_trainer_pc_term(*args) == -1 and b"image" in err(), i
    for i, v in ((7, 0.0), (8, 0.0), (7, float("nan")), (8, float("inf")), (5, float("nan")), (6, float("inf"))):
        args = list(ok)
        args[i] = v
        assert L.sdfr_vae_trainer_pc_term(*args) == -1 and b"intrinsics" in err(), i
    args = list(ok)
    args[15] = float("nan")
    assert L.sdfr_vae_trainer_pc_term(*args) == -1 and b"pc_weight" in err()
    for i in (1, 9, 10, 11, 12, 13, 16, 17, 18):
        args = list(ok)
        args[i] = None
        assert L.sdfr_vae_trainer_pc_term(*args) == -2 and b"sdfr_vae_trainer_pc_term: NULL pointer" in err(), i
    args = list(ok)
    args[19] = None
    assert L.sdfr_vae_trainer_pc_term(*args) == -2 and b"NULL workspace" in err()
    args = list(ok)
    args[20] = 100
    assert L.sdfr_vae_trainer_pc_term(*args) == -3 and b"sdfr_vae_trainer_pc_term: workspace 100 <" in err()
    # the workspace: an int64 volume per sample and the term's records; a function of its own
    one, two = (L.sdfr_vae_trainer_pc_term_workspace_bytes(h, n) for n in (1, 2))
    assert one >= 16 ** 3 * 8 and two - one >= 16 ** 3 * 8
    assert L.sdfr_vae_trainer_pc_term_workspace_bytes(None, 2) == 0 and L.sdfr_vae_trainer_pc_term_workspace_bytes(h, 0) == 0
    L.sdfr_vae_trainer_destroy(h)
    # the orientations
    assert L.sdfr_vae_trainer_pc_orientations(5, -1, q, 0, None) == -1 and b"sdfr_vae_trainer_pc_orientations: N=-1" in err()
    assert L.sdfr_vae_trainer_pc_orientations(5, 70000, q, 0, None) == -1
    assert L.sdfr_vae_trainer_pc_orientations(5, 2, None, 0, None) == -2 and b"NULL quat" in err()
    assert L.sdfr_vae_trainer_pc_orientations(5, 0, None, 0, None) == 0        # nothing to do


def test_workspace_of_the_other_calls_keeps_its_values():
    """sdfr_vae_trainer_workspace_bytes is not the term's: the mug at N = 2 and N = 8 as the parent commit sized it"""
    from sdfest_amd import _lib
    L = _lib.lib()
    h = create(L, tw.mug_setup()[0])
    sizes = [L.sdfr_vae_trainer_workspace_bytes(h, n) for n in (2, 8)]
    pc = [L.sdfr_vae_trainer_pc_term_workspace_bytes(h, n) for n in (2, 8)]
    L.sdfr_vae_trainer_destroy(h)
    assert pc == [n * 64 ** 3 * 8 + n * 128 * 4 + 256 for n in (2, 8)]
    assert sizes == [17150464, 68598528]
