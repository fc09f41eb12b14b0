"""Decoders other than the mug's that the render-and-compare loop can run on, and a float64 statement of the loop's
first iteration for any decoder (tests/test_loop_decoders_cpu.py, tests/test_loop_decoders_gpu.py).

The code that differs per decoder INSIDE the loop (csrc/loop.hip loop_tail_kernel with csrc/decoder_fc.hpp's
fc_stack_backward_one_wave / fc_narrow_forward_one_wave / fc_wide_slice / fc_stack_backward_sample, Adam over 8 + L
parameters, and pipeline.py's choice of the form) is reached with the shapes of FAMILY below: the smallest ones that take
each path.  Random weights give no volume a sphere tracer can use, so every decoder is built to put out

    a sphere SDF  +  a small field that depends on the latent:

  * channel 0 of the LAST Linear layer has zero weights and a bias that holds the sphere SDF on the s^3 grid, shifted by
    SHIFT (every Linear layer is ReLU'd: the shift keeps the values positive);
  * every convolution passes channel 0 through its centre tap; the last one's bias takes the shift off again;
  * everything else is a seeded normal draw -- the convolutions' scaled by EPS -- with biases that keep most units of the
    leading Linear layers alive (a chain of seven random narrow layers is dead otherwise: d/d latent exactly 0).

Nothing here comes from the reference: the weights are draws of the seeds below.  Every number a scene hands to the GPU
is rounded to float32 first, so the float64 statement and the kernels start from the same values.
"""
import functools
import json
import os

import numpy as np
import torch

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
FLOORS_PATH = os.path.join(HERE, "golden", "loop_decoder_floors.json")

EPS, SHIFT, RADIUS = 0.05, 2.0, 0.55
W, H, F = 64, 48, 60.0
THRESHOLD, DEPTH_WEIGHT, PC_WEIGHT = 0.005, 1.0, 3.0
GROUPS = (("position", slice(0, 3)), ("orientation", slice(3, 7)), ("scale", slice(7, 8)), ("latent", slice(8, None)))

# name -> latent, hidden widths of the leading Linear layers, channels and size the first convolution enters at, volume,
# the weights' seed and the scene's (chosen when this file was written: the first scene seed whose three scenes meet
# the conditions that tests/test_loop_decoders_cpu.py asserts -- `measures` below).  `narrow`: what
# sdfr_decoder_fc_one_wave must say.
FAMILY = {
    # n_fc = 1: no leading layer (span 0, a[n_fc - 1] is the latent); 432 outputs = 2 workgroups, the second 176 of 256
    "one_layer": dict(latent=5, hidden=[], channels=2, s=6, volume=16, seed=1, scene_seed=1, narrow=True),
    # layer inputs of exactly 64 lanes; span 6110 with or without the alignment gaps: the 4th staging round, partly
    "edge64": dict(latent=64, hidden=[64, 30], channels=2, s=6, volume=16, seed=1, scene_seed=1, narrow=True),
    # weights + biases 6080 floats, with the gaps of the device image 6176 > 6144: NOT one wave
    "gap": dict(latent=63, hidden=[63, 32], channels=2, s=6, volume=16, seed=1, scene_seed=4, narrow=False),
    # n_fc = 8 (the last rows of FcWaveLds::a); 250 outputs: one partial workgroup
    "deep8": dict(latent=3, hidden=[7, 5, 9, 4, 6, 8, 5], channels=2, s=5, volume=16, seed=1, scene_seed=17, narrow=True),
    # a hidden width above 64: fc_stack_backward_sample in the tail by nature; R = 32, 3 channels
    "wide": dict(latent=12, hidden=[70], channels=3, s=6, volume=32, seed=1, scene_seed=0, narrow=False),
    # n_params = 256, the tail's limit: every thread owns a parameter; a latent wider than a wave
    "latent248": dict(latent=248, hidden=[20], channels=2, s=6, volume=16, seed=1, scene_seed=4, narrow=False),
}
NAMES = tuple(FAMILY)
# construction only: 8 + 249 = 257 parameters, one more than the one-workgroup tails take
OVERSIZE = dict(latent=249, hidden=[20], channels=2, s=6, volume=16, seed=1, scene_seed=0, narrow=False)


# ---- quaternions (x, y, z, w), Adam, and the pose-only loop of tests/test_pipeline_gpu.py ------------------------------

def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def qinv(q):
    return q * np.array([-1, -1, -1, 1.0])


def qrot(q, v):
    return qmul(qmul(q, np.append(v, 0.0)), qinv(q))[:3]


def left_mul_matrix(a):
    """M with qmul(a, b) = M @ b."""
    ax, ay, az, aw = a
    return np.array([[aw, -az, ay, ax], [az, aw, -ax, ay], [-ay, ax, aw, az], [-ax, -ay, -az, aw]])


class NumpyAdam:
    def __init__(self, lrs):
        self.lrs, self.m, self.v, self.t = lrs, [0.0] * len(lrs), [0.0] * len(lrs), 0

    def step(self, params, grads):
        self.t += 1
        out = []
        for i, (p, g) in enumerate(zip(params, grads)):
            self.m[i] = 0.9 * self.m[i] + 0.1 * g
            self.v[i] = 0.999 * self.v[i] + 0.001 * g * g
            mh = self.m[i] / (1 - 0.9 ** self.t)
            vh = self.v[i] / (1 - 0.999 ** self.t)
            out.append(p - self.lrs[i] * mh / (np.sqrt(vh) + 1e-8))
        return out


def view_terms(sdf, depth_image, cloud, cam_pos, cam_quat, p, nq, s, cam, thr, wd, wpc, dtype=np.float64,
               with_sdf_grad=False):
    """One view of simple_setup.py:411-446 and its backward through the oracle: the gradients w.r.t. the object's
    position, its NORMALISED orientation and its scale in the world frame (and, with_sdf_grad, w.r.t. the volume), the
    estimate's depth image and the two loss values."""
    Wd, Hd, fx, fy, cx, cy = cam
    qw2c = qinv(cam_quat)
    Rw2c = np.stack([qrot(qw2c, e) for e in np.eye(3)], axis=1)
    pc = Rw2c @ (p - cam_pos)
    qc = qmul(qw2c, nq)
    est = oracle.render_forward(sdf, pc, qc, [1.0 / s], Wd, Hd, cx, cy, fx, fy, thr, dtype=dtype)[0]
    mask = (depth_image > 0) & (est > 0)
    gimg = wd * np.sign(est - depth_image) * mask / mask.sum()
    g_sdf, g_pc, g_qc, g_is = oracle.render_backward(gimg, est, sdf, pc, qc, [1.0 / s], cx, cy, fx, fy, dtype=dtype)
    val = oracle.pc_loss_forward(cloud, pc, qc, s, sdf, dtype=dtype)
    go = wpc * np.sign(val) / len(val)
    g_sdf2, g_pc2, g_qc2, g_s2 = oracle.pc_loss_backward(go, cloud, pc, qc, s, sdf, dtype=dtype)
    out = dict(g_p=Rw2c.T @ (g_pc[0].astype(np.float64) + g_pc2), g_nq=left_mul_matrix(qw2c).T @ (g_qc[0].astype(np.float64) + g_qc2),
               g_s=-float(g_is[0]) / s ** 2 + float(g_s2), est=est,
               loss_depth=float(np.abs(est - depth_image)[mask].mean()) if mask.any() else float("nan"),
               loss_pc=float(np.abs(val).mean()))
    if with_sdf_grad:
        out["g_sdf"] = g_sdf.astype(np.float64) + g_sdf2
    return out


def oracle_loop(sdf, depth_images, cam, cam_pos, cam_quat, p, q, s, thr, iters, wd, wpc):
    """numpy float64 restatement of simple_setup.py:408-462 with shape_optimization=False."""
    Wd, Hd, fx, fy, cx, cy = cam
    V = depth_images.shape[0]
    clouds = [oracle.depth_to_pointcloud(d, fx, fy, cx - 0.5, cy - 0.5, dtype=np.float64) for d in depth_images]
    adam = NumpyAdam([1e-3, 1e-2, 1e-3])
    traj = []
    for _ in range(iters):
        nq = q / np.linalg.norm(q)
        gp, gnq, gs = np.zeros(3), np.zeros(4), 0.0
        for v in range(V):
            t = view_terms(sdf, depth_images[v], clouds[v], cam_pos[v], cam_quat[v], p, nq, s, cam, thr, wd, wpc)
            gp += t["g_p"]
            gnq += t["g_nq"]
            gs += t["g_s"]
        n = np.linalg.norm(q)
        gq = (gnq - nq * (nq @ gnq)) / n
        p, q, s = adam.step([p, q, np.array(s)], [gp, gq, np.array(gs)])
        s = float(s)
        q = q / np.linalg.norm(q)
        traj.append((p.copy(), q.copy(), s))
    return traj


# ---- the decoders ------------------------------------------------------------------------------------------------------

def layers(spec):
    """(fc_layers, conv_layers) in the reference's config form"""
    C, s, vol = spec["channels"], spec["s"], spec["volume"]
    fc = [{"out": int(h)} for h in spec["hidden"]] + [{"out": C * s ** 3}]
    conv = [dict(in_size=s, in_channels=C, out_channels=C, kernel_size=3, relu=True),
            dict(in_size=vol // 2 + 2, in_channels=C, out_channels=1, kernel_size=3, relu=False)]
    return fc, conv


def config(spec):
    fc, conv = layers(spec)
    return {"latent_size": spec["latent"], "tsdf": False, "sdf_size": spec["volume"],
            "decoder": {"fc_layers": fc, "conv_layers": conv}}


def sphere_on_grid(s):
    """the sphere SDF at the cell centres of an s^3 grid over [-1, 1]^3"""
    g = (np.arange(s) + 0.5) / s * 2 - 1
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    return np.sqrt(X ** 2 + Y ** 2 + Z ** 2) - RADIUS


def state_dict(spec):
    """float32 parameters under the reference's names (decoder._fc_layers.{i}.weight ...)"""
    rng = np.random.default_rng(spec["seed"])
    fc, conv = layers(spec)
    C, s = spec["channels"], spec["s"]
    st = {}
    w = spec["latent"]
    for i, l in enumerate(fc):
        st[f"decoder._fc_layers.{i}.weight"] = (rng.normal(size=(l["out"], w)) / np.sqrt(w)).astype(np.float32)
        # (leading layers: most units alive at any latent of the scenes, some not -- the ReLU masks matter)
        last = i == len(fc) - 1
        st[f"decoder._fc_layers.{i}.bias"] = ((0.0 if last else 0.25) + 0.1 * rng.normal(size=l["out"])).astype(np.float32)
        w = l["out"]
    last = len(fc) - 1
    Wl = st[f"decoder._fc_layers.{last}.weight"].reshape(C, s ** 3, -1)
    Bl = st[f"decoder._fc_layers.{last}.bias"].reshape(C, s ** 3)
    Wl[0] = 0.0
    Bl[0] = (sphere_on_grid(s) + SHIFT).ravel()
    for i, l in enumerate(conv):
        k, ci, co = l["kernel_size"], l["in_channels"], l["out_channels"]
        wt = (EPS * rng.normal(size=(co, ci, k, k, k)) / np.sqrt(ci * k ** 3)).astype(np.float32)
        b = (EPS * rng.normal(size=co)).astype(np.float32)
        wt[0, 0] = 0.0
        wt[0, 0, k // 2, k // 2, k // 2] = 1.0          # channel 0 passes through
        if i == 0:
            wt[1:, 0] = 0.0                             # (and reaches no other channel)
            b[0] = 0.0
        if i == len(conv) - 1:
            b[0] = -SHIFT
        st[f"decoder._conv_layers.{i}.weight"] = wt
        st[f"decoder._conv_layers.{i}.bias"] = b
    return st


def spec_of(name):
    return FAMILY[name] if isinstance(name, str) else name


def decode(name, z, dtype=torch.float64):
    """(N, 1, R, R, R) torch tensor of `dtype` on the CPU, differentiable w.r.t. z: tests/test_decoder_gpu.py's plain
    statement of SDFDecoder.forward"""
    from test_decoder_gpu import torch_decoder
    spec = spec_of(name)
    fc, conv = layers(spec)
    return torch_decoder(state_dict(spec), fc, conv, spec["volume"], z, dtype=dtype)


def gpu_decoder(name):
    from sdfest_amd import SDFDecoder
    spec = spec_of(name)
    return SDFDecoder.from_config(config(spec), state_dict(spec), sdf_size=spec["volume"])


# ---- the scenes --------------------------------------------------------------------------------------------------------

CAMERA = (W, H, F, F, W / 2, H / 2)                      # tests/test_pipeline_gpu.py::test_iteration_matches_numpy_restatement
_f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)


def _cameras():
    cq = np.array([0.02, 0.27, 0.01, 1.0])
    cq /= np.linalg.norm(cq)
    return _f32([[0.0, 0.0, 0.0], [0.25, 0.05, 0.02]]), _f32(np.stack([np.array([0.0, 0, 0, 1.0]), cq]))


def _observe(name, z_true, p_true, q_true, s_true, cam_pos, cam_quat):
    with torch.no_grad():
        sdf = decode(name, torch.tensor(z_true[None]))[0, 0].numpy()
    obs = []
    for cp, cq in zip(cam_pos, cam_quat):
        qw2c = qinv(cq)
        obs.append(oracle.render_forward(sdf, qrot(qw2c, p_true - cp), qmul(qw2c, q_true / np.linalg.norm(q_true)),
                                         [1 / s_true], W, H, W / 2, H / 2, F, F, THRESHOLD, dtype=np.float64)[0])
    return _f32(np.stack(obs))


@functools.lru_cache(maxsize=None)
def _scenes(name, scene_seed):
    spec = FAMILY[name]
    rng = np.random.default_rng([scene_seed, spec["latent"]])
    L = spec["latent"]
    cam_pos, cam_quat = _cameras()
    out = {}
    # "views": one estimate seen by 2 cameras.  "object0" / "object1": the two estimates of the multi-object loop, one
    # view each from the camera at the origin -- object 0 is the first view of "views"
    for k, (p_true, q_true, s_true) in enumerate([([0.01, -0.015, -0.45], [0.3, 0.5, -0.1, 0.8], 0.11),
                                                  ([-0.02, 0.012, -0.5], [-0.4, 0.2, 0.3, 0.7], 0.1)]):
        p_true, q_true = _f32(p_true), np.array(q_true)
        q_true = _f32(q_true / np.linalg.norm(q_true))
        z_true = _f32(0.5 * rng.normal(size=L))
        z0 = _f32(z_true + 0.15 * rng.normal(size=L))
        p0 = _f32(p_true + np.array([0.008, -0.006, 0.01]) * (1 - 2 * k))
        q0 = _f32(q_true + np.array([0.04, -0.03, 0.02, 0.01]))
        s0 = float(np.float32(s_true * (1.09 - 0.15 * k)))
        obs = _observe(name, z_true, p_true, q_true, float(np.float32(s_true)), cam_pos, cam_quat)
        sc = dict(name=name, z_true=z_true, p0=p0, q0=q0, s0=s0, z0=z0)
        if k == 0:
            out["views"] = dict(sc, obs=obs, cam_pos=cam_pos, cam_quat=cam_quat)
        out[f"object{k}"] = dict(sc, obs=obs[:1], cam_pos=cam_pos[:1], cam_quat=cam_quat[:1])
    return out


def scene(name, which="views", scene_seed=None):
    """dict(name, obs (V,H,W), cam_pos, cam_quat, p0, q0, s0, z0, z_true): float64 arrays of float32-exact values"""
    return _scenes(name, FAMILY[name]["scene_seed"] if scene_seed is None else scene_seed)[which]


SCENES = ("views", "object0", "object1")


# ---- the first iteration, for any decoder -------------------------------------------------------------------------------

def first_iteration(sc, dtype=np.float64, margins=False):
    """simple_setup.py:408-456 for the scene's first estimate with shape optimisation: the vector
    [position 3 | orientation 4 | scale 1 | latent L] of d loss / d parameter BEFORE Adam, in float64 (oracle float64,
    float64 decoder) or -- the FLOOR -- float32 (oracle float32, float32 decoder).  d loss / d SDF is summed over the
    views from oracle.render_backward and oracle.pc_loss_backward; d loss / d latent comes by autograd through the plain
    decoder.  Returns dict(grads, est (V,H,W), loss_depth (V,), loss_pc (V,), sdf[, margin (V,H,W)])."""
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    _, _, fx, fy, cx, cy = CAMERA
    z = torch.tensor(sc["z0"][None], dtype=tdt, requires_grad=True)
    sdf_t = decode(sc["name"], z, dtype=tdt)[0, 0]
    sdf = sdf_t.detach().numpy()
    p, q, s = sc["p0"], sc["q0"], sc["s0"]
    n = np.linalg.norm(q)
    nq = q / n
    gp, gnq, gs, g_sdf = np.zeros(3), np.zeros(4), 0.0, np.zeros(sdf.shape)
    est, ld, lp, mar = [], [], [], []
    for v in range(sc["obs"].shape[0]):
        cloud = oracle.depth_to_pointcloud(sc["obs"][v], fx, fy, cx - 0.5, cy - 0.5, dtype=dtype)
        t = view_terms(sdf, sc["obs"][v].astype(dtype), cloud, sc["cam_pos"][v], sc["cam_quat"][v], p, nq, s, CAMERA,
                       THRESHOLD, DEPTH_WEIGHT, PC_WEIGHT, dtype=dtype, with_sdf_grad=True)
        gp += t["g_p"]
        gnq += t["g_nq"]
        gs += t["g_s"]
        g_sdf += t["g_sdf"]
        est.append(t["est"])
        ld.append(t["loss_depth"])
        lp.append(t["loss_pc"])
        if margins:
            qw2c = qinv(sc["cam_quat"][v])
            oracle.set_margin_mode(True)
            try:
                mar.append(oracle.render_forward(sdf, qrot(qw2c, p - sc["cam_pos"][v]), qmul(qw2c, nq), [1.0 / s], W, H, cx,
                                                 cy, fx, fy, THRESHOLD, dtype=dtype, with_aux=True)[2][0])
            finally:
                oracle.set_margin_mode(False)
    (sdf_t * torch.tensor(g_sdf, dtype=tdt)).sum().backward()
    gq = (gnq - nq * (nq @ gnq)) / n
    out = dict(grads=np.concatenate([gp, gq, [gs], z.grad[0].numpy().astype(np.float64)]), est=np.stack(est),
               loss_depth=np.array(ld), loss_pc=np.array(lp), sdf=sdf)
    if margins:
        out["margin"] = np.stack(mar)
    return out


def measures(sc):
    """what the conditions on a scene are stated in: per view the hit pixels of the float64 first estimate, its overlap
    with the observation, the smallest hit-test margin (oracle.set_margin_mode(True)), whether the float32 pass renders
    the same hit mask; and how far the latent moves the volume, max |sdf(z0) - sdf(0)|"""
    r64 = first_iteration(sc, np.float64, margins=True)
    r32 = first_iteration(sc, np.float32)
    hit = r64["est"] > 0
    with torch.no_grad():
        flat = decode(sc["name"], torch.zeros((1, len(sc["z0"])), dtype=torch.float64))[0, 0].numpy()
    return dict(hits=hit.sum(axis=(1, 2)), observed=(sc["obs"] > 0).sum(axis=(1, 2)),
                overlap=(hit & (sc["obs"] > 0)).sum(axis=(1, 2)),
                min_margin=np.array([np.abs(m).min() for m in r64["margin"]]),
                same_mask=np.array([np.array_equal(a > 0, b > 0) for a, b in zip(r64["est"], r32["est"])]),
                latent_moves=float(np.abs(r64["sdf"] - flat).max()), grads=r64["grads"],
                floor=group_distance(r32["grads"], r64["grads"]))


def meets_conditions(m):
    return bool(m["hits"].min() >= 300 and m["observed"].min() >= 300 and m["overlap"].min() >= 200
                and m["min_margin"].min() >= 2e-7 and m["same_mask"].all() and m["latent_moves"] >= 1e-3
                and np.count_nonzero(m["grads"][8:]) >= 0.75 * len(m["grads"][8:]))


def group_scale(g):
    """per entry: the largest component of the entry's group (tests/test_loop_g7_gpu.py::test_first_gradient_matches_g7)"""
    g = np.asarray(g, dtype=np.float64)
    return np.concatenate([np.full(len(g[sl]), np.abs(g[sl]).max()) for _, sl in GROUPS])


def group_distance(got, ref):
    """[position, orientation, scale, latent]: the largest |got - ref| of the group over the group's largest |ref|"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref) / group_scale(ref)
    return np.array([err[sl].max() for _, sl in GROUPS])


@functools.lru_cache(maxsize=None)
def reference(name, which="views"):
    """the float64 first iteration of a committed scene (computed once per process, shared, never modified)"""
    out = first_iteration(scene(name, which), np.float64)
    for v in out.values():
        v.setflags(write=False)
    return out


def compute_floor(name, which="views"):
    """float32 against float64, per group: what the number format alone costs on this scene"""
    return group_distance(first_iteration(scene(name, which), np.float32)["grads"], reference(name, which)["grads"])


def committed_floors():
    with open(FLOORS_PATH) as f:
        return json.load(f)


def bound(name, which="views"):
    """per group: max(1e-4, 10 x floor) -- 1e-4 of a group's largest component is the yardstick on a clean scene
    (test_first_gradient_matches_g7, scene C), 10 x the float32 floor the margin for a summation order that is not the
    reference's (tests/test_init_train_gpu.py)"""
    return np.maximum(1e-4, 10.0 * np.array(committed_floors()[name][which]))
