"""The architectures, batches and option settings the VAE decoder (sdfest_amd/csrc/decoder.hip, decoder_plan.hpp) is
walked over, for tests/test_decoder_cases_cpu.py (the cases are what they claim to be) and tests/test_decoder_edges_gpu.py
(every planned launch form and VJP entry point against float64).  Everything here runs on the CPU, in torch.

``CATALOGUE`` holds hand-written edges: each names the SDFR_DECODER_STEP_* forms (``SDFDecoder.STEPS`` names) it exists to
reach, and together they sit on both sides of the planner's thresholds.  ``case("seed 3")`` adds a seeded random draw.

A case is kept only where a comparison against float64 means something (``conditions``): (a) no ReLU pre-activation lies
within 4x torch fp32's deviation from float64 of 0 (DESIGN 3.13's margin), (b) torch fp32 on the CPU stays within 1e-5 of
float64 on every compared tensor, in units of its largest float64 entry, (c) every ReLU'd layer has at least 1% of its
values on each side, (d) no compared gradient is identically zero.  Weights, latents and upstream gradients come from a
sub-draw; the first of ``SUB_DRAWS`` that meets the conditions with ``HEADROOM`` on each of ``CPU_PATHS`` is the one
committed in tests/golden/decoder_case_floors.json (``python tests/decoder_cases.py`` rewrites it), with the fp32 floors
of this process.  Never reads the reference."""
import collections
import contextlib
import functools
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))

MARGIN = 4.0             # a ReLU input must lie this many times torch fp32's deviation from 0
FLOOR = 1e-5             # largest accepted fp32 floor, of each tensor's largest float64 entry
SIDES = 0.01             # smallest share of a ReLU'd layer's values on either side of 0
MAX_RELU_VALUES = 250000  # ReLU inputs of a case (N included): beyond, few sub-draws keep every one clear of 0
MAX_DRAW_MACS = 20000000  # convolution multiply-adds of a random draw: its sub-draws' search stays within seconds on one CPU thread
SUB_DRAWS = 20
HEADROOM = 1.5
CPU_PATHS = ({}, {"MKL_ENABLE_INSTRUCTIONS": "AVX2", "ATEN_CPU_CAPABILITY": "avx2"},
             {"MKL_ENABLE_INSTRUCTIONS": "SSE4_2", "ATEN_CPU_CAPABILITY": "default"})
FLOORS = os.path.join(HERE, "golden", "decoder_case_floors.json")
SCALED_VIEWS = (1, 2, 7, 64)   # the view counts of sdfr_decoder_backward_latent_deferred_scaled the tests run


def arch(latent, fc, conv, volume, N, tsdf=False, opts=None, forms=()):
    """fc: the hidden widths (the wide layer is added); conv: (in_size, in_channels, out_channels, kernel_size, relu)"""
    conv = [dict(in_size=a, in_channels=b, out_channels=c, kernel_size=k, relu=bool(r)) for a, b, c, k, r in conv]
    fc = [{"out": o} for o in fc] + [{"out": conv[0]["in_channels"] * conv[0]["in_size"] ** 3}]
    return dict(latent=latent, fc=fc, conv=conv, volume=volume, N=N, tsdf=tsdf, opts=dict(opts or {}), forms=set(forms))


# the smallest shapes that take each form; which form a layer takes is decoder_plan.hpp's (cited by function)
_SINGLE = dict(latent=4, fc=[16], conv=[(6, 5, 6, 3, 1),        # 6^3 x 5 channels (135 taps: split-K), -> 4
                                         (12, 6, 3, 3, 1),       # 4 -> 12 (a 3x resize) -> 10
                                         (20, 3, 1, 1, 0)],      # swapped 1x1x1 (3 -> 1 channels), 10 -> 20 = the volume
               volume=20)
_FC65 = dict(latent=65, fc=[70], conv=[(4, 4, 3, 1, 1),          # a 1x1x1 layer that is not swapped (4^3 = 64 voxels)
                                       (8, 3, 1, 3, 0)],         # 4 -> 8 -> 6
             volume=8)
_FINE32 = dict(latent=3, fc=[20], conv=[(5, 2, 4, 3, 1),         # -> 3
                                        (32, 4, 4, 3, 0),        # 3 -> 32 (fine size 32, 30^3: 30 direct tiles) -> 30
                                        (30, 4, 1, 1, 0)],
               volume=24)                                        # 30 -> 24: a down-sizing final resize
_RESIDENT = dict(latent=5, fc=[], conv=[(7, 4, 17, 3, 0),        # 17 channels: two column tiles; 5^3 outputs (8 rows)
                                        (5, 17, 1, 1, 0)],
                 volume=8)
CATALOGUE = {
    # one latent, the default options: the resize in the split-K MFMA operand fetch with the swapped layer in its
    # epilogue (mfma_up), the VJP's first stage fused with the transposed resize + 3-channel mix (vjp_stage, which adds
    # the scaled volumes on load), the one-wave Linear stack both ways
    "single_default": arch(**_SINGLE, N=1, forms={"fc_stack_narrow", "mfma_split_k", "mfma_up", "resize", "vjp_stage",
                                                  "resize_t_tiled", "fc_last_t", "fc_stack_t_wave"}),
    # the same without the fused pairs and without the tiled transposed resizes: z + y, x with the 3-channel mix, x with
    # mask + padding; the scaled form's sum is a launch of its own
    "single_unfused_untiled": arch(**_SINGLE, N=1, opts=dict(fused_single=0, tiled_vjp=0),
                                   forms={"resize_t_zy", "resize_t_x_mix_pad", "resize_t_x_pad", "mfma", "resize_mix",
                                          "scaled_combine"}),
    # every fused pair (bits 2 and 8 too) at the largest batch that keeps them (SDFR_SPLITK_MAX_LATENTS = 16) ...
    "fused_all_n16": arch(**_SINGLE, N=16, opts=dict(fused_single=15), forms={"fc_conv", "mfma_up", "vjp_stage"}),
    # ... and one latent past it: none of them, the plain MFMA forms; the one-wave Linear stack switched off
    "fused_all_n17": arch(**_SINGLE, N=17, opts=dict(fused_single=15, fc_one_wave=0),
                          forms={"fc_stack", "mfma", "resize_t_tiled", "fc_stack_t"}),
    # a kernel size of 5, a swapped 1x1x1 layer that mixes 4 channels into 2 (resize3_mix_kernel forward; the x pass
    # with the mix in the VJP), a ReLU on the last layer (its taped output is copied out), a tsdf clamp
    "mix_4_to_2_k5_relu_last": arch(3, [12], [(7, 3, 4, 5, 1),       # 7 -> 3
                                                (9, 4, 2, 1, 0),        # swapped 4 -> 2, 3 -> 9
                                                (12, 2, 1, 3, 1)],      # 9 -> 12 -> 10 = the volume, ReLU'd
                                      volume=10, N=2, tsdf=0.3,
                                      forms={"resize_mix", "resize_t_x_mix_pad", "resize_t_zy", "copy", "clamp",
                                             "mfma_split_k", "pad_mask"}),
    # a swapped layer past the mix limit (5 output channels: its own MFMA launch and a resize behind it), tsdf = True
    "swap_6_to_5_clamp": arch(4, [], [(4, 6, 6, 3, 1), (8, 6, 5, 1, 1), (8, 5, 1, 3, 0)], volume=6, N=4, tsdf=True,
                              forms={"mfma", "resize", "resize_t_tiled", "copy", "clamp", "pad_mask"}),
    # a Linear layer input of 65 (not the one-wave form), a hidden width over 64; N = 31 / 32: the batch forms of the
    # Linear stack (4 x kFcSamples), of the wide layer's transpose and of the 1x1x1 convolution
    "fc65_n31": arch(**_FC65, N=31, forms={"fc_stack", "conv1x1", "fc_last_t", "fc_stack_t"}),
    "fc65_n32": arch(**_FC65, N=32, forms={"fc_stack_batch", "conv1x1_vec4", "fc_last_t_batch", "fc_stack_t"}),
    # a one-layer Linear stack at N = 128: the resize 4 -> 16 folded into the direct convolution (fine size 16, the
    # default fused_resize = 1), the tiled forward resize, the direct transposed convolution, a 1-channel layer
    "fine16_n128": arch(3, [], [(4, 2, 1, 1, 1), (16, 1, 8, 3, 0), (14, 8, 1, 1, 0)], volume=16, N=128,
                        forms={"fc_stack_batch_narrow", "conv1x1_vec4", "direct_up", "resize_tiled", "fc_last_t_batch",
                               "resize_t_tiled", "fc_stack_t_wave"}),
    # N = 8 / 7 on a layer of 30 tiles (SDFR_DIRECT_MIN_LATENTS_FEW): fine size 32 folded (fused_resize = 2), unfolded
    # (0: the tiled resize and the direct convolution), and one latent short of the direct forms
    "fine32_n8_folded": arch(**_FINE32, N=8, opts=dict(fused_resize=2),
                             forms={"direct_up", "direct", "resize", "resize_t_zy", "resize_t_axis"}),
    "fine32_n8_unfolded": arch(**_FINE32, N=8, opts=dict(fused_resize=0), forms={"resize_tiled", "direct"}),
    "fine32_n7": arch(**_FINE32, N=7, opts=dict(fused_resize=2), forms={"resize_tiled", "mfma"}),
    # fine size 64 with 16 output channels (248 tiles: 3 latents reach 512 workgroups); 2 -> 64 spans more than the
    # z + y launch and the tiled form take: three single-axis passes in the VJP
    "fine64_n3": arch(2, [], [(4, 1, 1, 3, 1), (64, 1, 16, 3, 0), (62, 16, 1, 1, 0)], volume=16, N=3,
                      opts=dict(fused_resize=2), forms={"direct_up", "resize_t_axis", "resize_t_x_pad"}),
    # m^2 (m / zg) N = 30^2 x 10 x 8 = 72000 >= 65536: the z-grouped MFMA (5 output channels, 3 z per group); fine32_n7
    # has the same 30^3 layer at 63000 below it
    "zgroup_n8": arch(3, [], [(6, 2, 3, 3, 1), (32, 3, 5, 3, 0), (30, 5, 1, 1, 0)], volume=30, N=8,
                      forms={"mfma_z_grouped", "resize_tiled", "conv1x1"}),
    # N x column tiles = 64 x 2 = 128: the MFMA form with its input resident in LDS; 63 x 2 below it; 17 channels
    "resident_17ch_n64": arch(**_RESIDENT, N=64, forms={"mfma_resident", "fc_stack_batch_narrow", "fc_last_t_batch"}),
    "resident_17ch_n63": arch(**_RESIDENT, N=63, forms={"mfma", "fc_stack_batch_narrow"}),
    # the one-wave Linear stack's 6144-float span: 64 -> 64 -> 30 lies in 6110 floats (one wave) ...
    "fc_span_fits": arch(64, [64, 30], [(3, 2, 4, 3, 1), (6, 4, 1, 3, 0)], volume=4, N=2,
                         forms={"fc_stack_narrow", "fc_stack_t_wave"}),
    # ... 63 -> 63 -> 32 in 6080 floats, 6176 with the 64-float alignment gaps of the device image (not one wave)
    "fc_span_gaps": arch(63, [63, 32], [(3, 2, 4, 3, 1), (6, 4, 1, 3, 0)], volume=4, N=2,
                         forms={"fc_stack", "fc_stack_t"}),
}
# step codes no public call reaches (code -> the decoder_plan.hpp line that excludes it); none so far
UNREACHABLE = {}


def step_names():
    """the SDFR_DECODER_STEP_* names of include/sdfr.h, as SDFDecoder.STEPS spells them"""
    from sdfest_amd import _lib
    return [k[len("SDFR_DECODER_STEP_"):].lower() for k in _lib.ABI if k.startswith("SDFR_DECODER_STEP_")]


def fc_wave_span(c):
    """floats from the first Linear layer's weights to the end of the last leading layer's bias in the device image
    (sdfr_decoder_create: every block starts 64-float aligned), as decoder_fc.hpp's fc_wave_span measures it"""
    off, w_off, b_off, width = 0, [], [], [c["latent"]] + [l["out"] for l in c["fc"]]
    for l in range(len(c["fc"])):
        off = (off + 63) // 64 * 64
        w_off.append(off)
        off = (off + width[l + 1] * width[l] + 63) // 64 * 64
        b_off.append(off)
        off += width[l + 1]
    last = len(c["fc"]) - 1
    return 0 if last < 1 else b_off[last - 1] + width[last] - w_off[0]


# ---- the seeded random draw -----------------------------------------------------------------------------------------
def draw(seed, attempt=0):
    """a seeded architecture, batch and option setting in the fuzz test's space (tests/test_decoder_fuzz_gpu.py)"""
    rng = np.random.default_rng([0xDEC0DE, seed, attempt])
    latent, n_fc, n_conv = int(rng.integers(1, 13)), int(rng.integers(1, 5)), int(rng.integers(2, 5))
    chans = [int(rng.integers(1, 25)) for _ in range(n_conv)] + [1]
    size = int(rng.integers(2, 7))
    fc = [int(rng.integers(3, 70)) for _ in range(n_fc - 1)]
    conv, cur = [], size
    for i in range(n_conv):
        k = int(rng.choice([1, 3, 3, 5])) if (i > 0 or size >= 5) else int(rng.choice([1, 3] if size >= 3 else [1]))
        in_size = max(size, k) if i == 0 else int(np.clip(cur + rng.integers(-1, 14), k, 34))
        if k == 5:
            chans[i] = min(chans[i], 7)
            if i + 1 < n_conv:
                chans[i + 1] = min(chans[i + 1], 7)
            if i > 0:
                conv[i - 1][2] = chans[i]
        conv.append([in_size, chans[i], chans[i + 1], k, bool(i < n_conv - 1 and rng.uniform() < 0.8)])
        cur = in_size - k + 1
    if rng.uniform() < 0.3:
        conv[-1][4] = True
    volume = int(np.clip(cur + rng.integers(-2, 12), 2, 40))
    tsdf = [False, False, 0.1, True][int(rng.integers(0, 4))]
    N = int(rng.choice([1, 1, 2, 5, 16, 17, 32, 48]))
    opts = dict(fused_resize=int(rng.integers(0, 3)), tiled_vjp=int(rng.integers(0, 2)),
                fc_one_wave=int(rng.uniform() < 0.8), fused_single=int(rng.integers(0, 16)))
    return arch(latent, fc, [tuple(c) for c in conv], volume, N, tsdf, opts)


def relu_values(c):
    """ReLU inputs of a forward over the case's N latents: every Linear layer's and every ReLU'd convolution's"""
    n = sum(l["out"] for l in c["fc"])
    n += sum(l["out_channels"] * (l["in_size"] - l["kernel_size"] + 1) ** 3 for l in c["conv"] if l["relu"])
    return c["N"] * n


def conv_macs(c):
    """multiply-adds of the forward's convolutions over the case's N latents"""
    return c["N"] * sum(l["out_channels"] * (l["in_size"] - l["kernel_size"] + 1) ** 3 * l["in_channels"] *
                        l["kernel_size"] ** 3 for l in c["conv"])


@functools.lru_cache(maxsize=None)
def architecture(seed):
    """the first draw of `seed` within MAX_RELU_VALUES and MAX_DRAW_MACS"""
    for attempt in range(50):
        c = draw(seed, attempt)
        if relu_values(c) <= MAX_RELU_VALUES and conv_macs(c) <= MAX_DRAW_MACS:
            return c
    raise AssertionError(f"seed {seed}: no draw within {MAX_RELU_VALUES} ReLU values and {MAX_DRAW_MACS} multiply-adds")


def spec(name):
    """the architecture of a catalogue entry or of a seed ("seed 3")"""
    return CATALOGUE[name] if name in CATALOGUE else architecture(int(name.split()[1]))


def describe(c):
    conv = [(l["in_size"], l["in_channels"], l["out_channels"], l["kernel_size"], int(l["relu"])) for l in c["conv"]]
    return (f"N={c['N']} latent={c['latent']} fc={[l['out'] for l in c['fc']]} conv={conv} volume={c['volume']} "
            f"tsdf={c['tsdf']} opts={c['opts']}")


# ---- one sub-draw: weights, latents, upstream gradients ---------------------------------------------------------------
def inputs(name, sub):
    """state dict, z [N][latent], G [N][1][D][D][D] and the scaled form's volumes (N = 1 only): float32 numpy"""
    c = spec(name)
    rng = np.random.default_rng([zlib.crc32(name.encode()), sub])
    state, width = {}, c["latent"]
    for i, l in enumerate(c["fc"]):
        state[f"decoder._fc_layers.{i}.weight"] = (rng.normal(size=(l["out"], width)) / np.sqrt(width)).astype(np.float32)
        state[f"decoder._fc_layers.{i}.bias"] = rng.normal(scale=0.1, size=l["out"]).astype(np.float32)
        width = l["out"]
    for i, l in enumerate(c["conv"]):
        k = l["kernel_size"]
        fan = l["in_channels"] * k ** 3
        state[f"decoder._conv_layers.{i}.weight"] = (rng.normal(
            size=(l["out_channels"], l["in_channels"], k, k, k)) / np.sqrt(fan)).astype(np.float32)
        state[f"decoder._conv_layers.{i}.bias"] = rng.normal(scale=0.1, size=l["out_channels"]).astype(np.float32)
    D, N = c["volume"], c["N"]
    z = rng.normal(size=(N, c["latent"])).astype(np.float32)
    G = rng.normal(size=(N, 1, D, D, D)).astype(np.float32)
    scaled = {}
    if N == 1:
        for n in SCALED_VIEWS:
            # grad_out + sum_v k_v grad_scaled[v], k_v = weight / count[v] (0 where count is 0): view 1 of several
            # has count 0 and holds values that must not reach the sum
            count = rng.integers(1, 9, size=n).astype(np.float32)
            parts = rng.normal(size=(n, D, D, D)).astype(np.float32)
            if n > 1:
                count[1] = 0.0
                parts[1] = 1e30
            g0 = (0.5 * rng.normal(size=(D, D, D))).astype(np.float32)
            scaled[n] = dict(grad_out=g0, parts=parts, count=count, weight=np.float32(0.75))
    return state, z, G, scaled


def scaled_sum(s):
    """float64 of grad_out + sum_v k_v grad_scaled[v]"""
    g = s["grad_out"].astype(np.float64).copy()
    for v, cnt in enumerate(s["count"]):
        if cnt > 0:
            g += (np.float64(s["weight"]) / np.float64(cnt)) * s["parts"][v].astype(np.float64)
    return g


# ---- the layers, written out -------------------------------------------------------------------------------------------
def walk(c, state, z, dtype):
    """the decoder layer by layer (the order of test_decoder_gpu.torch_decoder, which the CPU test holds it to bit for
    bit): (out, [pre-activation of every ReLU], h = the wide Linear layer's input (retains its grad), the last layer's
    output before its ReLU resized to the volume)"""
    P = lambda key: torch.tensor(state[key]).to(dtype)
    pres, out, h = [], z, z
    n_fc = len(c["fc"])
    for i in range(n_fc):
        if i == n_fc - 1:
            h = out
            if h.requires_grad and not h.is_leaf:
                h.retain_grad()
        pre = F.linear(out, P(f"decoder._fc_layers.{i}.weight"), P(f"decoder._fc_layers.{i}.bias"))
        pres.append(pre)
        out = F.relu(pre)
    conv = c["conv"]
    out = out.view(-1, conv[0]["in_channels"], *([conv[0]["in_size"]] * 3))
    last_pre = None
    for i, l in enumerate(conv):
        if out.shape[2] != l["in_size"]:
            out = F.interpolate(out, size=(l["in_size"],) * 3, mode="trilinear", align_corners=False)
        out = F.conv3d(out, P(f"decoder._conv_layers.{i}.weight"), P(f"decoder._conv_layers.{i}.bias"))
        if l["relu"]:
            pres.append(out)
            last_pre = out
            out = F.relu(out)
    volume = c["volume"]
    resize = lambda t: t if t.shape[2] == volume else F.interpolate(t, size=(volume,) * 3, mode="trilinear",
                                                                     align_corners=False)
    out = resize(out)
    pre_out = resize(last_pre) if conv[-1]["relu"] else None
    return out, pres, h, pre_out


def clamp_of(c):
    return None if c["tsdf"] is False else (1.0 if c["tsdf"] is True else float(c["tsdf"]))


def run(c, state, z, G, scaled, dtype, vjp=True):
    """forward and VJPs in `dtype`: out, the output yardstick, pres, g_z, t_mid, and per scaled view count t_mid"""
    zt = torch.tensor(z).to(dtype).requires_grad_(vjp)
    with torch.set_grad_enabled(vjp):
        out, pres, h, pre_out = walk(c, state, zt, dtype)
    r = {"out": out.detach().numpy(), "pres": [p.detach().numpy() for p in pres],
         "scale": float(np.abs((pre_out if pre_out is not None else out).detach().numpy()).max())}
    if not vjp:
        return r
    t = clamp_of(c)
    if t is not None:
        base = (pre_out if pre_out is not None else out).detach().numpy()
        r["clamp"], r["clamp_scale"] = np.clip(r["out"], -t, t), float(np.abs(np.clip(base, -t, t)).max())
    gz, tm = torch.autograd.grad(out, [zt, h], torch.tensor(G).to(dtype), retain_graph=True)
    r["g_z"], r["t_mid"] = gz.numpy(), tm.numpy()
    r["scaled"] = {}
    for n, s in scaled.items():
        g = torch.tensor(scaled_sum(s)).to(dtype).reshape(G.shape)
        (tm,) = torch.autograd.grad(out, [h], g, retain_graph=True)
        r["scaled"][n] = tm.numpy()
    return r


@contextlib.contextmanager
def one_thread():
    """one CPU thread: one summation order for the fp32 run on every machine"""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(before)


def rel(a, b, scale=None):
    scale = float(np.abs(b).max()) if scale is None else scale
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(scale, 1e-300))


Report = collections.namedtuple("Report", "margin floor sides dead")
Case = collections.namedtuple("Case", "name spec sub state z G scaled report reference")


def conditions(c, state, z, G, scaled):
    """-> (Report, the float64 run).  margin: the smallest |pre-activation| in units of MARGIN x torch fp32's largest
    deviation at that layer (>= 1: condition a); floor: fp32 against float64 per compared tensor (b); sides: the
    smallest share of a ReLU'd layer's values on either side of 0 (c); dead: compared gradients that are all zero (d)"""
    margin, sides = float("inf"), 1.0
    with one_thread():
        ref, f32 = (run(c, state, z, G, scaled, dtype, vjp=False) for dtype in (torch.float64, torch.float32))
        for p64, p32 in zip(ref["pres"], f32["pres"]):
            dev = float(np.abs(p32.astype(np.float64) - p64).max())
            low = float(np.abs(p64).min())
            margin = min(margin, low / (MARGIN * dev) if dev > 0 else (float("inf") if low > 0 else 0.0))
            pos = float((p64 > 0).mean())
            sides = min(sides, pos, 1.0 - pos)
        if margin < 1.0 or sides < SIDES:     # (a) or (c) fails: the VJPs are not worth running
            return Report(margin, None, sides, []), ref
        ref = run(c, state, z, G, scaled, torch.float64)
        f32 = run(c, state, z, G, scaled, torch.float32)
    floor = {"out": rel(f32["out"], ref["out"], ref["scale"]), "g_z": rel(f32["g_z"], ref["g_z"]),
             "t_mid": rel(f32["t_mid"], ref["t_mid"])}
    if "clamp" in ref:
        floor["clamp"] = rel(f32["clamp"], ref["clamp"], ref["clamp_scale"])
    if ref["scaled"]:
        floor["scaled"] = max(rel(f32["scaled"][n], ref["scaled"][n]) for n in ref["scaled"])
    dead = [k for k in ("g_z", "t_mid") if not np.abs(ref[k]).max() > 0]
    dead += [f"scaled {n}" for n, t in ref["scaled"].items() if not np.abs(t).max() > 0]
    return Report(margin, floor, sides, dead), ref


def accepted(r, room=1.0):
    return (r.floor is not None and not r.dead and r.margin >= room and r.sides >= SIDES
            and max(r.floor.values()) <= FLOOR / room)


def roomy(r):
    return accepted(r, HEADROOM)


def setup(name, sub):
    c = spec(name)
    state, z, G, scaled = inputs(name, sub)
    report, ref = conditions(c, state, z, G, scaled)
    return Case(name, c, sub, state, z, G, scaled, report, ref)


def search(name):
    """the first of SUB_DRAWS sub-draws that meets the conditions with HEADROOM on this machine's path, or None"""
    for sub in range(SUB_DRAWS):
        c = setup(name, sub)
        if roomy(c.report):
            return c
    return None


def default_seeds():
    return range(int(os.environ.get("SDFR_FUZZ_SEEDS", "16")))


def names():
    return list(CATALOGUE) + [f"seed {s}" for s in range(16)]


@functools.lru_cache(maxsize=None)
def load_table():
    with open(FLOORS) as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def case(name):
    """the case the committed table names (a seed beyond the table: the first sub-draw ``search`` picks here)"""
    entry = load_table().get(name)
    if entry is None:
        found = search(name)
        assert found is not None, f"{name}: none of {SUB_DRAWS} sub-draws meets the conditions"
        return found
    return setup(name, entry["sub"])


def floor_of(c):
    """the committed floors of a case (a seed beyond the table: the ones just measured)"""
    entry = load_table().get(c.name)
    assert entry is None or entry["sub"] == c.sub, c.name
    return entry["floor"] if entry else c.report.floor


def bound(c, tensor):
    """max(1e-4, 10 x the committed fp32 floor), in units of the tensor's largest float64 entry"""
    return max(1e-4, 10.0 * floor_of(c)[tensor])


# ---- the table -------------------------------------------------------------------------------------------------------
def compute_table():
    """name -> {sub, floor}: the first sub-draw that is ``roomy`` on this path and on the two other CPU_PATHS (a process
    each: the BLAS picks its instruction path when it loads), with the floors this process measures"""
    table = {}
    for name in names():
        for sub in range(SUB_DRAWS):
            c = setup(name, sub)
            if not roomy(c.report):
                continue
            ok = True
            for env in CPU_PATHS[1:]:
                done = subprocess.run([sys.executable, os.path.abspath(__file__), "--roomy", name, str(sub)],
                                      env=dict(os.environ, **env), capture_output=True, text=True, check=True)
                ok = ok and json.loads(done.stdout)
            if ok:
                table[name] = {"sub": sub, "floor": c.report.floor}
                print(name, sub, f"margin {c.report.margin:.2f}", {k: f"{v:.2e}" for k, v in c.report.floor.items()},
                      flush=True)
                break
        assert name in table, f"{name}: no sub-draw has room on every path"
    return table


if __name__ == "__main__":
    if sys.argv[1:2] == ["--roomy"]:
        print(json.dumps(roomy(setup(sys.argv[2], int(sys.argv[3])).report)))
        sys.exit(0)
    table = compute_table()
    with open(FLOORS, "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
        fh.write("\n")
