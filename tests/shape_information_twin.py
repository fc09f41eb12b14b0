"""float64 twin of the shape-uncertainty code (test-side only): the decoder's forward-mode derivative, the joint
pose-latent Gram matrix and the joint tangent information.  Nothing here imports the product.

Decoder JVP: ``torch.func.jvp`` through ``decoder_cases.walk`` (the layer walk the decoder tests hold to
test_decoder_gpu.torch_decoder) in float64; the same in float32 gives the floor a GPU bound is ten times of.

Latent features: d depth_pixel / d SDF is ``oracle.render_backward(one_hot(pixel), ..., dtype=float64,
sdf_grad_mode=0)`` -- the oracle the goldens pin --, contracted with the tangent volumes; one call per included pixel,
each writing a 64^3 float64 volume: measured here about 1.4 ms a pixel -- 0.4 s for the 280 included pixels of the scenes
the GPU test names, under 3 s for the pipeline test and its 2575 pixels (12 s when every call was handed the whole one-hot
image); the pixel is handed over as a 1 x 1 image, see ``pixel_sdf_gradient``.

Pose features: ``information_twin.features`` (``oracle.render_derivative_images``).

Run as a script, this file writes tests/golden/decoder_jvp_floors.json (the pattern of decoder_cases.py)."""
import functools
import json
import os
import sys
import zlib

import numpy as np
import torch

import decoder_cases as dc
import information_twin as twin
import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
JVP_FLOORS = os.path.join(GOLDEN, "decoder_jvp_floors.json")
# the catalogue cases of the JVP test (their committed sub-draws: no ReLU input near 0) and their tangent counts
JVP_CASES = ("single_default", "mix_4_to_2_k5_relu_last", "swap_6_to_5_clamp", "fc65_n31", "fine32_n8_folded",
             "resident_17ch_n63")
JVP_T = (1, 3)
MUG = "mug"        # the trained mug decoder of the goldens, the identity basis (T = 8), one latent


# ---- decoder JVP ------------------------------------------------------------------------------------------------------
def tangents(name, T):
    """seeded directions (N, T, latent) float32 of a catalogue case"""
    s = dc.spec(name)
    rng = np.random.default_rng([zlib.crc32(name.encode()), 0x4A5650, T])
    return rng.normal(size=(s["N"], T, s["latent"])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def mug():
    """(spec, state, z (1, 8)) of the mug decoder in decoder_cases' terms"""
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    w = np.load(os.path.join(GOLDEN, "mug_decoder_weights.npz"))
    state = {(k if k.startswith("decoder.") else "decoder." + k): w[k] for k in w.files}
    conv = [dict(in_size=int(a), in_channels=int(b), out_channels=int(c), kernel_size=int(k), relu=bool(r))
            for a, b, c, k, r in zip(d["conv_in_size"], d["conv_cin"], d["conv_cout"], d["conv_k"], d["conv_relu"])]
    spec = dict(latent=int(d["latent_size"]), fc=[{"out": int(o)} for o in d["fc_out"]], conv=conv, volume=64, N=1,
                tsdf=False, opts={}, forms=set())
    return spec, state, np.ascontiguousarray(d["z"][:1], dtype=np.float32)


def decoder_jvp(spec, state, z, tan, dtype):
    """(out (N,1,D,D,D), tangent volumes (N,T,D,D,D)) of the unclamped decoder in `dtype`, as numpy"""
    zt = torch.tensor(z).to(dtype)
    f = lambda v: dc.walk(spec, state, v, dtype)[0]
    rows, out = [], None
    with torch.no_grad():
        for t in range(tan.shape[1]):
            out, d = torch.func.jvp(f, (zt,), (torch.tensor(tan[:, t]).to(dtype),))
            rows.append(d[:, 0])
    return out.numpy(), torch.stack(rows, dim=1).numpy()


def jvp_inputs(name, T):
    """(spec, state, z, tangents or None for the identity basis) of a JVP case"""
    if name == MUG:
        spec, state, z = mug()
        assert T == spec["latent"]
        return spec, state, z, None
    c = dc.case(name)
    return c.spec, c.state, c.z, tangents(name, T)


@functools.lru_cache(maxsize=None)
def jvp_reference(name, T):
    """float64 (out, tangent volumes)"""
    spec, state, z, tan = jvp_inputs(name, T)
    tan = np.broadcast_to(np.eye(spec["latent"], dtype=np.float32), (len(z), T, T)) if tan is None else tan
    with dc.one_thread():
        return decoder_jvp(spec, state, z, tan, torch.float64)


def row_error(got, ref):
    """worst row (n, t) of max |got - ref| / max |ref|: the share of the tangent volume's largest float64 entry"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    axes = tuple(range(2, ref.ndim))
    scale = np.abs(ref).max(axis=axes)
    assert (scale > 0).all(), "a tangent volume that is identically zero"
    return float((np.abs(got - ref).max(axis=axes) / scale).max())


def jvp_floor(name, T):
    """torch fp32 against float64 (one thread)"""
    spec, state, z, tan = jvp_inputs(name, T)
    tan = np.broadcast_to(np.eye(spec["latent"], dtype=np.float32), (len(z), T, T)) if tan is None else tan
    with dc.one_thread():
        f32 = decoder_jvp(spec, state, z, tan, torch.float32)[1]
    return row_error(f32, jvp_reference(name, T)[1])


def jvp_case_ids():
    return [(n, T) for n in JVP_CASES for T in JVP_T] + [(MUG, 8)]


@functools.lru_cache(maxsize=None)
def load_jvp_floors():
    with open(JVP_FLOORS) as fh:
        return json.load(fh)


def jvp_bound(name, T):
    """max(1e-4, 10 x the committed fp32 floor), in units of the tangent volume's largest float64 entry"""
    return max(1e-4, 10.0 * load_jvp_floors()[name][f"T{T}"])


# ---- the joint Gram matrix ----------------------------------------------------------------------------------------------
MAX_T = 22


@functools.lru_cache(maxsize=None)
def tangent_fields(R=64, seed=5):
    """(22, R, R, R) float64, exactly representable in float32: seeded smooth fields (four low-frequency waves each)"""
    rng = np.random.default_rng(seed)
    x = np.linspace(-1.0, 1.0, R)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    out = np.zeros((MAX_T, R, R, R))
    for t in range(MAX_T):
        for _ in range(4):
            k = rng.uniform(-4.0, 4.0, size=3)
            out[t] += rng.normal() * np.sin(k[0] * X + k[1] * Y + k[2] * Z + rng.uniform(0, 2 * np.pi))
    return out.astype(np.float32).astype(np.float64)


def jac_buffer(fields, T):
    """the first T fields in the voxel-major layout (R^3, Tp) float32, zero padding"""
    R = fields.shape[-1]
    buf = np.zeros((R ** 3, (T + 3) & ~3), np.float32)
    buf[:, :T] = fields[:T].reshape(T, -1).T
    return buf


def pixel_sdf_gradient(depth, sdf, p, q, inv_scale, cx, cy, fx, fy, r, c, whole_image=False):
    """(R^3,) float64: d depth[r, c] / d SDF from the oracle's backward fed the one-hot image of that pixel.  The
    backward treats every pixel on its own, so the one-hot image is handed over as the 1 x 1 image of that pixel with
    the principal point moved by (c, r) -- the same ray and depth without a walk over the other pixels;
    ``whole_image=True`` hands over the full one-hot image (the CPU test holds the two to each other)."""
    d32 = np.asarray(depth, np.float32)
    if whole_image:
        g = np.zeros(d32.shape)
        g[r, c] = 1.0
        args = (g, d32, sdf, p, q, [inv_scale], cx, cy, fx, fy)
    else:
        args = (np.ones((1, 1)), d32[r:r + 1, c:c + 1], sdf, p, q, [inv_scale], cx - c, cy - r, fx, fy)
    return oracle.render_backward(*args, dtype=np.float64, sdf_grad_mode=0)[0].reshape(-1)


def latent_features(depth, sdf, p, q, inv_scale, cx, cy, fx, fy, inc, fields):
    """(H,W,T') float64: d depth / d (field t) of the included pixels -- the float64 oracle's d depth / d SDF of each
    pixel (exact trilinear weights), contracted with the fields"""
    H, W = np.shape(depth)
    flat = fields.reshape(len(fields), -1)
    s = np.zeros((H, W, len(fields)))
    threads = oracle.max_threads()
    oracle.set_threads(1)      # one pixel per call: a thread team per call costs more than the call (an earlier test of
    try:                       # the session may have asked for 64 threads)
        for r, c in np.argwhere(inc):
            g_sdf = pixel_sdf_gradient(depth, sdf, p, q, inv_scale, cx, cy, fx, fy, r, c)
            nz = np.flatnonzero(g_sdf)
            s[r, c] = flat[:, nz] @ g_sdf[nz]
    finally:
        oracle.set_threads(threads)
    return s


def joint_features(f10, s, T):
    """(H,W,10+T): (d0 .. d7, s0 .. s_{T-1}, r, 1) from information_twin.features' image and latent_features'"""
    return np.concatenate([f10[..., :8], s[..., :T], f10[..., 8:]], axis=-1)


def joint_tangent_information(g, q, inv_scale, cam_quat=None):
    """(7+T, 7+T) from a joint Gram matrix (10+T, 10+T): information_twin.tangent_map on the pose block, the identity
    on the latent block"""
    g = np.asarray(g, np.float64)
    L = g.shape[0] - 10
    M = np.zeros((8 + L, 7 + L))
    M[:8, :7] = twin.tangent_map(q, inv_scale, cam_quat)
    M[8:, 7:] = np.eye(L)
    H = M.T @ g[:8 + L, :8 + L] @ M
    return 0.5 * (H + H.T)


if __name__ == "__main__":
    table = {}
    for name, T in jvp_case_ids():
        table.setdefault(name, {})[f"T{T}"] = jvp_floor(name, T)
        print(name, T, f"{table[name][f'T{T}']:.2e}", flush=True)
    with open(JVP_FLOORS, "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
        fh.write("\n")
