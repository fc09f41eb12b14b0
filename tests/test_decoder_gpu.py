"""GPU: the HIP VAE decoder against the golden outputs of the reference's SDFDecoder (mug weights)
and against the oracle."""
import os

import numpy as np
import pytest
import torch

import oracle
from helpers import GOLDEN, decoder_probe_G

pytestmark = pytest.mark.gpu


def mug_config(d):
    return {"latent_size": int(d["latent_size"]), "tsdf": False, "decoder": {
        "fc_layers": [{"out": int(o)} for o in d["fc_out"]],
        "conv_layers": [{"in_size": int(a), "in_channels": int(b), "out_channels": int(c),
                         "kernel_size": int(k), "relu": bool(r)}
                        for a, b, c, k, r in zip(d["conv_in_size"], d["conv_cin"], d["conv_cout"],
                                                 d["conv_k"], d["conv_relu"])]}}


@pytest.fixture(scope="module")
def mug():
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    w = np.load(os.path.join(GOLDEN, "mug_decoder_weights.npz"))
    return d, {k: w[k] for k in w.files}


def test_mug_decoder_matches_reference_golden(mug):
    from sdfest_amd import SDFDecoder
    d, w = mug
    dec = SDFDecoder.from_config(mug_config(d), w)
    z = torch.tensor(d["z"], device="cuda")
    with torch.no_grad():
        out = dec.decode(z)
    assert out.shape == (12, 1, 64, 64, 64)
    o = out.cpu().numpy()
    ref0 = d["z0_full"]
    assert np.max(np.abs(o[0, 0] - ref0)) <= 1e-4 * np.max(np.abs(ref0))
    for i in range(12):
        sub = d["sub16"][i]
        assert np.max(np.abs(o[i, 0, ::4, ::4, ::4] - sub)) <= 1e-4 * max(1.0, np.abs(sub).max())
        s = d["stats"][i]
        assert abs(o[i].sum(dtype=np.float64) - s[0]) <= 1e-4 * s[1]
    # batched == one at a time, bit for bit while the kernels keep the single decode's form (fewer than 8 latents);
    # from 8 latents on the layers of many tiles take the direct convolution (round 5: the K objects of a frame side by
    # side) and agree to rounding, like a large batch (test_batched_decoder_kernels_equal_single_decodes)
    with torch.no_grad():
        one = dec.decode(z[5:6])
        few = dec.decode(z[:7])
    assert torch.equal(one[0], few[5])
    assert (one[0] - out[5]).abs().max().item() <= 2e-5 * max(one.abs().max().item(), 1e-3)


def test_decoder_matches_oracle_on_other_architectures():
    """Random weights, shapes that exercise: Cout > 16 (two channel tiles), k=1 mid-network,
    no final resize, a final resize, tsdf clamping, K not a multiple of 4."""
    from sdfest_amd import SDFDecoder
    rng = np.random.default_rng(0)
    cases = [
        dict(volume=16, latent=5, tsdf=0.1,
             fc=[{"out": 12}, {"out": 3 * 4 ** 3}],
             conv=[dict(in_size=4, in_channels=3, out_channels=20, kernel_size=3, relu=True),
                   dict(in_size=9, in_channels=20, out_channels=6, kernel_size=1, relu=True),
                   dict(in_size=12, in_channels=6, out_channels=1, kernel_size=3, relu=False)]),
        dict(volume=8, latent=3, tsdf=False,
             fc=[{"out": 2 * 5 ** 3}],
             conv=[dict(in_size=5, in_channels=2, out_channels=5, kernel_size=3, relu=True),
                   dict(in_size=10, in_channels=5, out_channels=1, kernel_size=3, relu=False)]),
        # batches: the direct convolution with 8 and 4 output channels on odd sizes (its scalar path, z runs
        # that end inside a 4-chunk) ...
        dict(volume=11, latent=3, tsdf=False, batch=150,
             fc=[{"out": 16 * 4 ** 3}],
             conv=[dict(in_size=4, in_channels=16, out_channels=16, kernel_size=3, relu=True),
                   dict(in_size=11, in_channels=16, out_channels=8, kernel_size=3, relu=True),
                   dict(in_size=13, in_channels=8, out_channels=4, kernel_size=3, relu=True),
                   dict(in_size=11, in_channels=4, out_channels=1, kernel_size=1, relu=False)]),
        # ... and on sizes that are multiples of 4 (its 16-byte path), with a final resize
        dict(volume=12, latent=3, tsdf=False, batch=160,
             fc=[{"out": 4 * 8 ** 3}],
             conv=[dict(in_size=8, in_channels=4, out_channels=8, kernel_size=3, relu=True),
                   dict(in_size=12, in_channels=8, out_channels=4, kernel_size=3, relu=True),
                   dict(in_size=10, in_channels=4, out_channels=1, kernel_size=1, relu=False)]),
    ]
    for case in cases:
        state = {}
        width = case["latent"]
        for i, l in enumerate(case["fc"]):
            state[f"decoder._fc_layers.{i}.weight"] = rng.normal(size=(l["out"], width)).astype(np.float32) / np.sqrt(width)
            state[f"decoder._fc_layers.{i}.bias"] = rng.normal(size=l["out"]).astype(np.float32) * 0.1
            width = l["out"]
        for i, l in enumerate(case["conv"]):
            k = l["kernel_size"]
            fan = l["in_channels"] * k ** 3
            state[f"decoder._conv_layers.{i}.weight"] = rng.normal(
                size=(l["out_channels"], l["in_channels"], k, k, k)).astype(np.float32) / np.sqrt(fan)
            state[f"decoder._conv_layers.{i}.bias"] = rng.normal(size=l["out_channels"]).astype(np.float32) * 0.1
        cfg = {"latent_size": case["latent"], "tsdf": case["tsdf"], "sdf_size": case["volume"],
               "decoder": {"fc_layers": case["fc"], "conv_layers": case["conv"]}}
        dec = SDFDecoder.from_config(cfg, state, sdf_size=case["volume"])
        z = rng.normal(size=(case.get("batch", 3), case["latent"])).astype(np.float32)
        params = oracle.pack_decoder_params(state, len(case["fc"]), len(case["conv"]))
        for enforce in (False, True):
            ref = oracle.decoder_forward(params, cfg, z, dtype=np.float32, enforce_tsdf=enforce)
            with torch.no_grad():
                out = dec.forward(torch.tensor(z, device="cuda"), enforce_tsdf=enforce).cpu().numpy()
            assert out.shape == ref.shape
            assert np.max(np.abs(out - ref)) <= 1e-4 * max(np.abs(ref).max(), 1e-3), case["volume"]
            if enforce and case["tsdf"]:
                assert np.abs(out).max() <= case["tsdf"] + 1e-7


def test_decoder_feeds_renderer(mug):
    """decode(z) -> render: the SDFPipeline hand-off (simple_setup.py:413-434), no host copy."""
    from sdfest_amd import Camera, SDFDecoder, render_depth_gpu
    d, w = mug
    dec = SDFDecoder.from_config(mug_config(d), w)
    with torch.no_grad():
        sdf = dec.decode(torch.zeros(1, 8, device="cuda"))
    cam = Camera(160, 120, 80.0, 80.0, 80.0, 60.0, pixel_center=0.5)
    p = torch.tensor([0.0, 0.0, -0.3], device="cuda")
    q = torch.tensor([0.0, 0.0, 0.0, 1.0], device="cuda")
    depth = render_depth_gpu(sdf[0, 0], p, q, torch.tensor(1 / 0.1, device="cuda"), None, None, None,
                             0.005, cam)
    ref = oracle.render_forward(d["z0_full"], [0, 0, -0.3], [0, 0, 0, 1], [10.0], 160, 120, 80.0, 60.0,
                                80.0, 80.0, 0.005, dtype=np.float32)[0]
    dd = depth.cpu().numpy()
    assert (ref > 0).sum() > 1000
    agree = (dd > 0) == (ref > 0)
    assert agree.mean() > 0.999
    both = (dd > 0) & (ref > 0)
    assert np.max(np.abs(dd[both] / ref[both] - 1)) < 1e-3   # the two SDFs differ by fp32 rounding


def test_decoder_latent_gradient_matches_torch_autograd_golden(mug):
    """d(sum(out * G))/dz for 12 latents against torch autograd through the reference decoder."""
    from helpers import decoder_probe_G
    from sdfest_amd import SDFDecoder
    d, w = mug
    G = decoder_probe_G()
    assert np.allclose(G[::4, ::4, ::4], d["G_sub16"], atol=1e-6)
    dec = SDFDecoder.from_config(mug_config(d), w)
    z = torch.tensor(d["z"], device="cuda", requires_grad=True)
    out = dec.decode(z)
    (out[:, 0] * torch.tensor(G, device="cuda")).sum().backward()
    gz = z.grad.cpu().numpy()
    # the north star's bound, 1e-4 of each latent's largest component, against the reference module in FLOAT64
    # (tools/make_goldens.py::make_decoder, vae.double()) ...
    ref = d["grad_z_f64"]
    scale = np.abs(ref).max(axis=1, keepdims=True)
    err = np.max(np.abs(gz - ref) / scale)
    assert err <= 1e-4, f"latent gradient vs the float64 reference decoder: {err:.2e} of the row maximum"
    # ... and 2e-4 only against the module's own float32 run: two fp32 implementations, each within its rounding of
    # the float64 value (the torch one by 9e-7 here)
    ref32 = d["grad_z"]
    err32 = np.max(np.abs(gz - ref32) / np.abs(ref32).max(axis=1, keepdims=True))
    assert err32 <= 2e-4, f"latent gradient vs the fp32 torch run (fp32 against fp32): {err32:.2e}"
    # forward with a tape gives the same output as the inference path
    with torch.no_grad():
        assert torch.equal(dec.decode(z.detach()), out.detach())
    # linearity in the upstream gradient and one-at-a-time == batched
    z1 = torch.tensor(d["z"][9:10], device="cuda", requires_grad=True)
    o1 = dec.decode(z1)
    (o1[:, 0] * torch.tensor(G, device="cuda") * 2.0).sum().backward()
    assert np.allclose(z1.grad.cpu().numpy()[0], 2.0 * gz[9], rtol=1e-5, atol=1e-5 * scale[9])


def torch_decoder(state, fc, conv, volume, z, dtype=torch.float64):
    """Plain PyTorch (CPU, float64 unless `dtype` says float32) statement of SDFDecoder.forward (sdf_vae.py:217-259)."""
    import torch.nn.functional as F
    P = lambda name: torch.tensor(state[name]).to(dtype)
    out = z
    for i in range(len(fc)):
        out = F.relu(F.linear(out, P(f"decoder._fc_layers.{i}.weight"), P(f"decoder._fc_layers.{i}.bias")))
    out = out.view(-1, conv[0]["in_channels"], *([conv[0]["in_size"]] * 3))
    for i, l in enumerate(conv):
        if out.shape[2] != l["in_size"]:
            out = F.interpolate(out, size=(l["in_size"],) * 3, mode="trilinear", align_corners=False)
        out = F.conv3d(out, P(f"decoder._conv_layers.{i}.weight"), P(f"decoder._conv_layers.{i}.bias"))
        if l["relu"]:
            out = F.relu(out)
    if out.shape[2] != volume:
        out = F.interpolate(out, size=(volume,) * 3, mode="trilinear", align_corners=False)
    return out


def test_decoder_latent_gradient_other_architecture_vs_torch():
    """Architecture with Cout > 16 (two channel tiles forward, two in the data-gradient), k=1
    mid-network and a final resize: forward and VJP against a plain PyTorch float64 reference."""
    from sdfest_amd import SDFDecoder
    rng = np.random.default_rng(1)
    fc = [{"out": 12}, {"out": 3 * 4 ** 3}]
    conv = [dict(in_size=4, in_channels=3, out_channels=20, kernel_size=3, relu=True),
            dict(in_size=9, in_channels=20, out_channels=6, kernel_size=1, relu=True),
            dict(in_size=12, in_channels=6, out_channels=1, kernel_size=3, relu=False)]
    state, width = {}, 5
    for i, l in enumerate(fc):
        state[f"decoder._fc_layers.{i}.weight"] = rng.normal(size=(l["out"], width)).astype(np.float32) / np.sqrt(width)
        state[f"decoder._fc_layers.{i}.bias"] = rng.normal(size=l["out"]).astype(np.float32) * 0.1
        width = l["out"]
    for i, l in enumerate(conv):
        k = l["kernel_size"]
        state[f"decoder._conv_layers.{i}.weight"] = rng.normal(
            size=(l["out_channels"], l["in_channels"], k, k, k)).astype(np.float32) / np.sqrt(l["in_channels"] * k ** 3)
        state[f"decoder._conv_layers.{i}.bias"] = rng.normal(size=l["out_channels"]).astype(np.float32) * 0.1
    cfg = {"latent_size": 5, "tsdf": False, "decoder": {"fc_layers": fc, "conv_layers": conv}}
    dec = SDFDecoder.from_config(cfg, state, sdf_size=16)
    G = rng.normal(size=(16, 16, 16)).astype(np.float32)
    z0 = rng.normal(size=(3, 5)).astype(np.float32)
    z = torch.tensor(z0, device="cuda", requires_grad=True)
    out = dec.decode(z)
    (out[:, 0] * torch.tensor(G, device="cuda")).sum().backward()
    zt = torch.tensor(z0, dtype=torch.float64, requires_grad=True)
    ref = torch_decoder(state, fc, conv, 16, zt)
    (ref[:, 0] * torch.tensor(G).double()).sum().backward()
    assert np.max(np.abs(out.detach().cpu().numpy() - ref.detach().numpy())) <= 1e-4 * ref.abs().max().item()
    g, gr = z.grad.cpu().numpy(), zt.grad.numpy()
    assert np.max(np.abs(g - gr)) <= 1e-4 * np.abs(gr).max(), (g, gr)      # (gr: torch in float64)


def test_decoder_latent_gradient_wide_hidden_layer_vs_torch():
    """The transposed wide Linear layer runs one workgroup per (hidden unit, sample): with a hidden
    width of 2048 and 6 samples that is 12 288 workgroups, several times what is resident at once, so
    late workgroups read the layer's input gradient long after early ones have stored their results.
    (Round-1 advice: the results used to be stored into that same buffer.)  Against PyTorch float64."""
    from sdfest_amd import SDFDecoder
    rng = np.random.default_rng(2)
    fc = [{"out": 2048}, {"out": 2 * 6 ** 3}]
    conv = [dict(in_size=6, in_channels=2, out_channels=4, kernel_size=3, relu=True),
            dict(in_size=8, in_channels=4, out_channels=1, kernel_size=1, relu=False)]
    state, width = {}, 7
    for i, l in enumerate(fc):
        state[f"decoder._fc_layers.{i}.weight"] = rng.normal(size=(l["out"], width)).astype(np.float32) / np.sqrt(width)
        state[f"decoder._fc_layers.{i}.bias"] = rng.normal(size=l["out"]).astype(np.float32) * 0.1
        width = l["out"]
    for i, l in enumerate(conv):
        k = l["kernel_size"]
        state[f"decoder._conv_layers.{i}.weight"] = rng.normal(
            size=(l["out_channels"], l["in_channels"], k, k, k)).astype(np.float32) / np.sqrt(l["in_channels"] * k ** 3)
        state[f"decoder._conv_layers.{i}.bias"] = rng.normal(size=l["out_channels"]).astype(np.float32) * 0.1
    cfg = {"latent_size": 7, "tsdf": False, "decoder": {"fc_layers": fc, "conv_layers": conv}}
    dec = SDFDecoder.from_config(cfg, state, sdf_size=8)
    N = 6
    G = rng.normal(size=(N, 8, 8, 8)).astype(np.float32)
    z0 = rng.normal(size=(N, 7)).astype(np.float32)
    zt = torch.tensor(z0, dtype=torch.float64, requires_grad=True)
    ref = torch_decoder(state, fc, conv, 8, zt)
    (ref[:, 0] * torch.tensor(G).double()).sum().backward()
    gr = zt.grad.numpy()
    for _ in range(5):   # a race shows up in some runs only
        z = torch.tensor(z0, device="cuda", requires_grad=True)
        out = dec.decode(z)
        (out[:, 0] * torch.tensor(G, device="cuda")).sum().backward()
        assert np.max(np.abs(out.detach().cpu().numpy() - ref.detach().numpy())) <= 1e-4 * ref.abs().max().item()
        g = z.grad.cpu().numpy()
        assert np.max(np.abs(g - gr)) <= 1e-4 * np.abs(gr).max(), (g, gr)      # (gr: torch in float64)


def test_batched_decoder_kernels_equal_single_decodes(mug):
    """A batch large enough for the batched kernels (direct convolutions, tiled resizes, the MFMA convolution with its
    input resident in LDS) against one-at-a-time decodes, which take the latency-oriented kernels: forward and VJP.
    (The z-grouped MFMA is not among them: the mug decoder's first layer, the only one left to the matrix cores at
    N = 130, takes the resident form.)"""
    from sdfest_amd import SDFDecoder
    d, wts = mug
    dec = SDFDecoder.from_config(mug_config(d), wts)
    N = 130
    # the batch takes the batched forms the docstring names, a single decode none of them
    batched = {"direct", "resize_tiled", "mfma_resident"}
    plans = {n: set(dec.launch_plan(n, tape=True)) | set(dec.launch_plan(n, vjp=True)) for n in (N, 1)}
    assert batched <= plans[N] and "mfma_z_grouped" not in plans[N], plans[N]
    assert not (batched | {"mfma_z_grouped"}) & plans[1], plans[1]
    rng = np.random.default_rng(11)
    z_np = np.concatenate([d["z"], rng.normal(size=(N - len(d["z"]), 8)).astype(np.float32)])
    G = torch.tensor(decoder_probe_G(), device="cuda")
    w = torch.tensor(rng.uniform(0.5, 1.5, N).astype(np.float32), device="cuda")
    z = torch.tensor(z_np, device="cuda", requires_grad=True)
    out = dec.decode(z)
    (out[:, 0] * G * w[:, None, None, None]).sum().backward()
    ref0 = d["z0_full"]
    picks = [0, 1, 7, 64, 129]
    for i in picks:
        zi = torch.tensor(z_np[i:i + 1], device="cuda", requires_grad=True)
        oi = dec.decode(zi)
        (oi[:, 0] * G * w[i]).sum().backward()
        a, b = out[i].detach(), oi[0].detach()
        assert (a - b).abs().max().item() <= 2e-5 * max(b.abs().max().item(), 1e-3), i
        ga, gb = z.grad[i], zi.grad[0]
        assert (ga - gb).abs().max().item() <= 2e-4 * gb.abs().max().item(), (
            "batched against single-latent kernels -- fp32 against fp32, hence 2e-4 and not the 1e-4 kept for float64 "
            "comparands", i, ga, gb)
    # and the golden output of the reference decoder for the first latent (z = 0 is d["z"][0]?)
    with torch.no_grad():
        o = dec.decode(torch.zeros(N, 8, device="cuda"))
    assert np.max(np.abs(o[N - 1, 0].cpu().numpy() - ref0)) <= 1e-4 * np.max(np.abs(ref0))


def _random_state(rng, case):
    state, width = {}, case["latent"]
    for i, l in enumerate(case["fc"]):
        state[f"decoder._fc_layers.{i}.weight"] = rng.normal(size=(l["out"], width)).astype(np.float32) / np.sqrt(width)
        state[f"decoder._fc_layers.{i}.bias"] = rng.normal(size=l["out"]).astype(np.float32) * 0.1
        width = l["out"]
    for i, l in enumerate(case["conv"]):
        k = l["kernel_size"]
        fan = l["in_channels"] * k ** 3
        state[f"decoder._conv_layers.{i}.weight"] = rng.normal(
            size=(l["out_channels"], l["in_channels"], k, k, k)).astype(np.float32) / np.sqrt(fan)
        state[f"decoder._conv_layers.{i}.bias"] = rng.normal(size=l["out_channels"]).astype(np.float32) * 0.1
    return state


def test_tiled_transposed_resize_is_bitwise_the_three_launches(mug):
    """Batched VJP: each transposed resize as ONE launch on an LDS-staged block (channel loop, register prefetch, fused
    mask / padding / swapped 1x1 layer) against the three single-axis launches (+ conv1x1 + pad_mask) it replaces --
    the same fmaf chains in the same order, so the latent gradients must agree bit for bit (single latents, whose
    captured loop takes the one-launch form too, included).  Shapes: the mug decoder
    (ratios 64/30, 32/14, 16/6; padded + masked, and the swapped last layer), up- and DOWN-sizing resizes, a coarse
    size that leaves a one-column tile, a channel count that is not a multiple of 8, 2 ... 4 mixed channels."""
    from sdfest_amd import SDFDecoder
    from sdfest_amd._lib import lib
    L = lib()
    d, wts = mug
    rng = np.random.default_rng(5)
    cases = [("mug", mug_config(d), wts, 64, 8, 70), ("mug", mug_config(d), wts, 64, 8, 1), ("mug", mug_config(d), wts, 64, 8, 3)]
    extra = [
        dict(volume=32, latent=4, batch=80, fc=[{"out": 3 * 6 ** 3}],
             conv=[dict(in_size=6, in_channels=3, out_channels=5, kernel_size=3, relu=True),      # -> 4
                   dict(in_size=13, in_channels=5, out_channels=3, kernel_size=3, relu=True),     # 4 -> 13 -> 11
                   dict(in_size=24, in_channels=3, out_channels=1, kernel_size=1, relu=False)]),  # 1x1, 11 -> 24 (swapped), -> 32
        dict(volume=40, latent=4, batch=80, fc=[{"out": 2 * 8 ** 3}],
             conv=[dict(in_size=8, in_channels=2, out_channels=6, kernel_size=1, relu=False),
                   dict(in_size=28, in_channels=6, out_channels=2, kernel_size=3, relu=True),     # 8 -> 28 (9 taps) -> 26
                   dict(in_size=24, in_channels=2, out_channels=1, kernel_size=3, relu=False)]),  # 26 -> 24 (down) -> 22 -> 40
        dict(volume=48, latent=3, batch=70, fc=[{"out": 4 * 5 ** 3}],
             conv=[dict(in_size=5, in_channels=4, out_channels=4, kernel_size=1, relu=True),
                   dict(in_size=20, in_channels=4, out_channels=2, kernel_size=3, relu=True),     # 5 -> 20 (11 taps) -> 18
                   dict(in_size=36, in_channels=2, out_channels=1, kernel_size=1, relu=False)]),  # 1x1, 18 -> 36 (swapped), -> 48
    ]
    for case in extra:
        cfg = {"latent_size": case["latent"], "tsdf": False, "sdf_size": case["volume"],
               "decoder": {"fc_layers": case["fc"], "conv_layers": case["conv"]}}
        cases.append((f"volume {case['volume']}", cfg, _random_state(rng, case), case["volume"], case["latent"], case["batch"]))
    for name, cfg, state, volume, latent, N in cases:
        dec = SDFDecoder.from_config(cfg, state, sdf_size=volume) if name != "mug" else SDFDecoder.from_config(cfg, state)
        z_np = rng.normal(size=(N, latent)).astype(np.float32)
        G = torch.tensor(rng.normal(size=(N, 1, volume, volume, volume)).astype(np.float32), device="cuda")
        grads = []
        for on in (1, 0):
            old = dec.set_option("tiled_vjp", on)
            try:
                plan = dec.launch_plan(N, vjp=True)
                if not on:
                    assert "resize_t_tiled" not in plan, (name, N, plan)
                elif name == "mug" and N in (70, 1):
                    assert "resize_t_tiled" in plan, (name, N, plan)
                z = torch.tensor(z_np, device="cuda", requires_grad=True)
                dec.decode(z).backward(G)
                torch.cuda.synchronize()
                grads.append(z.grad.clone())
            finally:
                dec.set_option("tiled_vjp", old)
        assert torch.isfinite(grads[0]).all() and grads[0].abs().max() > 0, name
        assert torch.equal(grads[0], grads[1]), (name, N, (grads[0] - grads[1]).abs().max().item())


def test_resize_folded_into_the_patch_load_is_bitwise_the_two_launches(mug):
    """Batched forward: an up-sampling trilinear resize in front of a 3x3x3 layer runs inside that layer's patch load
    (conv3d_direct_up_kernel: coarse columns staged in LDS, the fine patch formed with resize3_kernel's expression
    tree) against the resize launch + the direct convolution it replaces: outputs bit for bit, and the VJP through the
    taped forward as well.  Shapes: the mug decoder (6 -> 16 and 14 -> 32), a fine size of 64 (fewer patch-row slots
    than patch rows), 5 -> 16 and 7 -> 16, 16 output channels, channel counts that leave a short last chunk."""
    from sdfest_amd import SDFDecoder
    from sdfest_amd._lib import lib
    L = lib()
    d, wts = mug
    rng = np.random.default_rng(11)
    cases = [("mug", mug_config(d), wts, 64, 8, 140), ("mug", mug_config(d), wts, 64, 8, 20)]
    extra = [
        # (the first layer takes the Linear stack's output as it is, sdf_vae.py:207-215: resizes come after it)
        dict(volume=32, latent=4, batch=130, fc=[{"out": 5 * 5 ** 3}],
             conv=[dict(in_size=5, in_channels=5, out_channels=6, kernel_size=1, relu=True),      # 5^3
                   dict(in_size=16, in_channels=6, out_channels=16, kernel_size=3, relu=True),    # 5 -> 16 -> 14
                   dict(in_size=32, in_channels=16, out_channels=4, kernel_size=3, relu=True),    # 14 -> 32 -> 30
                   dict(in_size=30, in_channels=4, out_channels=1, kernel_size=1, relu=False)]),  # 1x1 (swapped) -> 32
        dict(volume=64, latent=3, batch=6, fc=[{"out": 2 * 11 ** 3}],
             conv=[dict(in_size=11, in_channels=2, out_channels=3, kernel_size=3, relu=True),     # 11 -> 9
                   dict(in_size=64, in_channels=3, out_channels=4, kernel_size=3, relu=False),    # 9 -> 64 -> 62
                   dict(in_size=62, in_channels=4, out_channels=1, kernel_size=1, relu=False)]),
        dict(volume=16, latent=5, batch=140, fc=[{"out": 3 * 7 ** 3}],
             conv=[dict(in_size=7, in_channels=3, out_channels=7, kernel_size=1, relu=False),     # 7^3
                   dict(in_size=16, in_channels=7, out_channels=8, kernel_size=3, relu=True),     # 7 -> 16 -> 14
                   dict(in_size=14, in_channels=8, out_channels=1, kernel_size=1, relu=False)]),
    ]
    for case in extra:
        cfg = {"latent_size": case["latent"], "tsdf": False, "sdf_size": case["volume"],
               "decoder": {"fc_layers": case["fc"], "conv_layers": case["conv"]}}
        cases.append((f"volume {case['volume']}", cfg, _random_state(rng, case), case["volume"], case["latent"], case["batch"]))
    for name, cfg, state, volume, latent, N in cases:
        dec = SDFDecoder.from_config(cfg, state, sdf_size=volume) if name != "mug" else SDFDecoder.from_config(cfg, state)
        z_np = rng.normal(size=(N, latent)).astype(np.float32)
        G = torch.tensor(rng.normal(size=(N, 1, volume, volume, volume)).astype(np.float32), device="cuda")
        outs, grads = [], []
        for on in (2, 0):      # folded wherever the form exists / never (the default folds fine sizes up to 16)
            old = dec.set_option("fused_resize", on)
            try:
                plan = dec.launch_plan(N, tape=True)
                if not on:
                    assert "direct_up" not in plan, (name, N, plan)
                elif name == "mug" and N == 140:
                    assert "direct_up" in plan, (name, N, plan)
                z = torch.tensor(z_np, device="cuda", requires_grad=True)
                o = dec.decode(z)
                o.backward(G)
                torch.cuda.synchronize()
                outs.append(o.detach().clone())
                grads.append(z.grad.clone())
            finally:
                dec.set_option("fused_resize", old)
        assert torch.isfinite(outs[0]).all() and outs[0].abs().max() > 0, name
        assert torch.equal(outs[0], outs[1]), (name, N, (outs[0] - outs[1]).abs().max().item())
        assert torch.equal(grads[0], grads[1]), (name, N)


def test_one_wave_linear_backward_is_bitwise_the_workgroup_form(mug):
    """The VJP's last launch for a narrow Linear stack (the mug decoder's 8 -> 20 -> 50 in front of the wide layer):
    one wave per latent with the weights staged in LDS (fc_stack_backward_wave_kernel) against the one-workgroup form
    that reloads them layer by layer -- the same fmaf chains, so the latent gradients agree bit for bit -- and the
    forward's stack of a single decode likewise (fc_stack_kernel<true>); a stack with a 70-wide layer does not qualify
    and must not be affected by the switch."""
    from sdfest_amd import SDFDecoder
    from sdfest_amd._lib import lib
    L = lib()
    d, wts = mug
    rng = np.random.default_rng(17)
    wide = dict(volume=32, latent=5, batch=3, fc=[{"out": 70}, {"out": 33}, {"out": 3 * 6 ** 3}],
                conv=[dict(in_size=6, in_channels=3, out_channels=4, kernel_size=3, relu=True),
                      dict(in_size=16, in_channels=4, out_channels=1, kernel_size=3, relu=False)])
    narrow = dict(volume=32, latent=64, batch=5, fc=[{"out": 64}, {"out": 7}, {"out": 64}, {"out": 2 * 5 ** 3}],
                  conv=[dict(in_size=5, in_channels=2, out_channels=3, kernel_size=3, relu=True),
                        dict(in_size=12, in_channels=3, out_channels=1, kernel_size=3, relu=False)])
    cases = [("mug", mug_config(d), wts, 64, 8, n) for n in (1, 3, 40)]
    for name, case in (("70 wide", wide), ("64 wide, four layers", narrow)):
        cfg = {"latent_size": case["latent"], "tsdf": False, "sdf_size": case["volume"],
               "decoder": {"fc_layers": case["fc"], "conv_layers": case["conv"]}}
        cases.append((name, cfg, _random_state(rng, case), case["volume"], case["latent"], case["batch"]))
    for name, cfg, state, volume, latent, N in cases:
        dec = SDFDecoder.from_config(cfg, state, sdf_size=volume) if name != "mug" else SDFDecoder.from_config(cfg, state)
        z_np = rng.normal(size=(N, latent)).astype(np.float32)
        G = torch.tensor(rng.normal(size=(N, 1, volume, volume, volume)).astype(np.float32), device="cuda")
        grads, outs = [], []
        for on in (1, 0):
            old = dec.set_option("fc_one_wave", on)
            try:
                plan = dec.launch_plan(N, tape=True) + dec.launch_plan(N, vjp=True)
                wave = {"fc_stack_t_wave", "fc_stack_narrow", "fc_stack_batch_narrow"} & set(plan)
                if not on or name == "70 wide":
                    assert not wave, (name, N, on, plan)
                elif name == "mug":
                    assert "fc_stack_t_wave" in wave, (name, N, plan)
                z = torch.tensor(z_np, device="cuda", requires_grad=True)
                o = dec.decode(z)
                o.backward(G)
                torch.cuda.synchronize()
                grads.append(z.grad.clone())
                outs.append(o.detach().clone())
            finally:
                dec.set_option("fc_one_wave", old)
        assert torch.isfinite(grads[0]).all() and grads[0].abs().max() > 0, name
        assert torch.equal(outs[0], outs[1]), (name, N, (outs[0] - outs[1]).abs().max().item())   # (the forward's stack too)
        assert torch.equal(grads[0], grads[1]), (name, N, (grads[0] - grads[1]).abs().max().item())


def _fused_single_cases(d, wts, rng):
    cases = [("mug", mug_config(d), wts, 64, 8, n) for n in (1, 3, 16)]
    extra = [
        # odd channel counts (padding taps), sizes that are no multiples of 4 (scalar rows of the wide layer), a 1x1x1
        # layer that is not swapped, a final resize behind the last layer
        dict(name="7 -> 5 | 12 -> 10 | 24 -> 22 | 1x1 | -> 32", volume=32, latent=4, batch=1, fc=[{"out": 3 * 7 ** 3}],
             conv=[dict(in_size=7, in_channels=3, out_channels=5, kernel_size=3, relu=True),
                   dict(in_size=12, in_channels=5, out_channels=3, kernel_size=3, relu=True),
                   dict(in_size=24, in_channels=3, out_channels=2, kernel_size=3, relu=True),
                   dict(in_size=22, in_channels=2, out_channels=1, kernel_size=1, relu=False)]),
        # a 5x resize (11 taps), three z tiles per column (46 and 48 rows), a swapped last layer with 4 mixed channels
        dict(name="6 -> 4 | 20 -> 18 | 48 -> 46 | swapped 1x1 -> 64", volume=64, latent=5, batch=2, fc=[{"out": 20}, {"out": 2 * 6 ** 3}],
             conv=[dict(in_size=6, in_channels=2, out_channels=4, kernel_size=3, relu=True),
                   dict(in_size=20, in_channels=4, out_channels=3, kernel_size=3, relu=True),
                   dict(in_size=48, in_channels=3, out_channels=4, kernel_size=3, relu=True),
                   dict(in_size=64, in_channels=4, out_channels=1, kernel_size=1, relu=False)]),
        # two column tiles of output channels (20), a layer without ReLU, two mixed channels
        dict(name="6 -> 4 (20 ch) | 12 -> 10 | swapped 1x1 -> 16", volume=16, latent=3, batch=2, fc=[{"out": 7}, {"out": 3 * 6 ** 3}],
             conv=[dict(in_size=6, in_channels=3, out_channels=20, kernel_size=3, relu=True),
                   dict(in_size=12, in_channels=20, out_channels=2, kernel_size=3, relu=False),
                   dict(in_size=16, in_channels=2, out_channels=1, kernel_size=1, relu=True)]),
        # an 8-wide first layer (16-byte rows of the wide layer) into a resize by 1 (none) and by 2
        dict(name="8 -> 6 | 6 -> 4 | 8 -> 6 | 1x1 -> 16", volume=16, latent=6, batch=5, fc=[{"out": 4 * 8 ** 3}],
             conv=[dict(in_size=8, in_channels=4, out_channels=6, kernel_size=3, relu=True),
                   dict(in_size=6, in_channels=6, out_channels=6, kernel_size=3, relu=True),
                   dict(in_size=8, in_channels=6, out_channels=3, kernel_size=3, relu=True),
                   dict(in_size=16, in_channels=3, out_channels=1, kernel_size=1, relu=False)]),
        # five channels into the first layer (135 taps: its split-K form, so the Linear stack folds into it), three mixed
        dict(name="7 (5 ch) -> 5 | 12 -> 10 | swapped 1x1 -> 16", volume=16, latent=4, batch=3, fc=[{"out": 12}, {"out": 5 * 7 ** 3}],
             conv=[dict(in_size=7, in_channels=5, out_channels=6, kernel_size=3, relu=True),
                   dict(in_size=12, in_channels=6, out_channels=3, kernel_size=3, relu=True),
                   dict(in_size=16, in_channels=3, out_channels=1, kernel_size=1, relu=False)]),
        # 18 output channels of the first layer (two column tiles) from 6 x 8^3, a 2.5x resize
        dict(name="8 (6 ch) -> 6 (18 ch) | 20 -> 18 | 1x1", volume=18, latent=7, batch=1, fc=[{"out": 33}, {"out": 6 * 8 ** 3}],
             conv=[dict(in_size=8, in_channels=6, out_channels=18, kernel_size=3, relu=True),
                   dict(in_size=20, in_channels=18, out_channels=2, kernel_size=3, relu=True),
                   dict(in_size=18, in_channels=2, out_channels=1, kernel_size=1, relu=False)]),
    ]
    for case in extra:
        cfg = {"latent_size": case["latent"], "tsdf": False, "sdf_size": case["volume"],
               "decoder": {"fc_layers": case["fc"], "conv_layers": case["conv"]}}
        cases.append((case["name"], cfg, _random_state(rng, case), case["volume"], case["latent"], case["batch"]))
    return cases


def test_single_latent_fused_pairs_are_bitwise_the_unfused_launches(mug):
    """Few latents (the render-and-compare loop decodes one): the layer PAIRS as one launch each -- the up-sampling
    resize inside the split-K MFMA convolution behind it (conv3d_mfma_up_kernel, sdf_vae.py:235-246), the Linear stack
    with the first convolution (fc_conv_kernel, :223-238), and in the VJP the transposed resize (+ mask, swapped 1x1x1
    layer, padding) inside the transposed convolution (vjp_stage_kernel: its first stage alone, bit 4, and the following
    stages chained to it through the z-pass epilogue, bits 4 + 8) -- against the launches they replace, every pair alone
    and all together (15): outputs, the taped activations the VJP reads, and the latent gradients bit for bit."""
    from sdfest_amd import SDFDecoder
    d, wts = mug
    rng = np.random.default_rng(23)
    for name, cfg, state, volume, latent, N in _fused_single_cases(d, wts, rng):
        dec = SDFDecoder.from_config(cfg, state, sdf_size=volume) if name == "mug" else SDFDecoder.from_config(cfg, state, sdf_size=volume)
        z_np = rng.normal(size=(N, latent)).astype(np.float32)
        G = torch.tensor(rng.normal(size=(N, 1, volume, volume, volume)).astype(np.float32), device="cuda")
        res = {}
        for bits in (0, 1, 2, 4, 12, 15):
            old = dec.set_option("fused_single", bits)
            try:
                plan = set(dec.launch_plan(N) + dec.launch_plan(N, tape=True) + dec.launch_plan(N, vjp=True))
                forms = {"mfma_up": 1, "fc_conv": 2, "vjp_stage": 4 | 8}
                for form, bit in forms.items():
                    if not bits & bit:
                        assert form not in plan, (name, N, bits, form)
                if name == "mug" and N == 1 and bits == 15:
                    assert set(forms) <= plan, (name, bits, plan)
                z = torch.tensor(z_np, device="cuda", requires_grad=True)
                o = dec.decode(z)
                o.backward(G)
                torch.cuda.synchronize()
                with torch.no_grad():
                    plain = dec.decode(torch.tensor(z_np, device="cuda"))   # (the forward without a tape)
                res[bits] = (o.detach().clone(), z.grad.clone(), plain.clone())
            finally:
                dec.set_option("fused_single", old)
        ref = res[0]
        assert torch.isfinite(ref[0]).all() and ref[0].abs().max() > 0 and ref[1].abs().max() > 0, name
        assert torch.equal(ref[0], ref[2]), name
        for bits in (1, 2, 4, 12, 15):
            o, g, plain = res[bits]
            assert torch.equal(o, ref[0]), (name, N, bits, "output", (o - ref[0]).abs().max().item())
            assert torch.equal(plain, ref[0]), (name, N, bits, "output without a tape", (plain - ref[0]).abs().max().item())
            assert torch.equal(g, ref[1]), (name, N, bits, "latent gradient", (g - ref[1]).abs().max().item())


def test_launch_plan_query():
    """sdfr_decoder_launch_plan on the smallest decoder of this file at N = 1 and 2: the same answer twice, a short
    `steps` array, the error codes, N = 0, and the stages of a forward (stage 1 + stage 2 launch what the whole forward
    launches, unless that one folds the Linear stack into the first convolution)."""
    import ctypes
    from sdfest_amd import SDFDecoder, _lib
    rng = np.random.default_rng(3)
    case = dict(volume=16, latent=3, fc=[{"out": 7}, {"out": 3 * 6 ** 3}],
                conv=[dict(in_size=6, in_channels=3, out_channels=20, kernel_size=3, relu=True),
                      dict(in_size=12, in_channels=20, out_channels=2, kernel_size=3, relu=False),
                      dict(in_size=16, in_channels=2, out_channels=1, kernel_size=1, relu=True)])
    cfg = {"latent_size": 3, "tsdf": False, "sdf_size": 16, "decoder": {"fc_layers": case["fc"], "conv_layers": case["conv"]}}
    dec = SDFDecoder.from_config(cfg, _random_state(rng, case), sdf_size=16)
    L, A = dec._L, _lib.ABI
    fwd, vjp = A["SDFR_DECODER_PASS_FORWARD"], A["SDFR_DECODER_PASS_VJP"]
    for N in (1, 2):
        for kw in (dict(), dict(tape=True), dict(vjp=True), dict(vjp=True, deferred=True)):
            plan = dec.launch_plan(N, **kw)
            assert plan and plan == dec.launch_plan(N, **kw), (N, kw)
        whole = dec.launch_plan(N, tape=True)
        if "fc_conv" not in whole:
            assert dec.launch_plan(N, tape=True, stages=1) + dec.launch_plan(N, tape=True, stages=2) == whole, N
        assert dec.launch_plan(N, vjp=True)[:-1] == dec.launch_plan(N, vjp=True, deferred=True), N
        # a short array: the full count, and only `capacity` entries written
        n = len(whole)
        steps = (ctypes.c_int * n)(*([-7] * n))
        assert n >= 3 and L.sdfr_decoder_launch_plan(dec._h, fwd, N, A["SDFR_DECODER_PLAN_TAPE"], steps, 2) == n
        assert [dec.STEPS[c] for c in steps[:2]] == whole[:2] and list(steps[2:]) == [-7] * (n - 2)
        assert L.sdfr_decoder_launch_plan(dec._h, fwd, N, A["SDFR_DECODER_PLAN_TAPE"], None, 0) == n
    steps = (ctypes.c_int * 64)()
    assert L.sdfr_decoder_launch_plan(None, fwd, 1, 0, steps, 64) == A["SDFR_E_NULL"]
    assert L.sdfr_decoder_launch_plan(dec._h, 2, 1, 0, steps, 64) == A["SDFR_E_INVALID"]
    assert L.sdfr_decoder_launch_plan(dec._h, fwd, 1, 128, steps, 64) == A["SDFR_E_INVALID"]
    assert L.sdfr_decoder_launch_plan(dec._h, fwd, 1, A["SDFR_DECODER_PLAN_DEFERRED"], steps, 64) == A["SDFR_E_INVALID"]
    assert L.sdfr_decoder_launch_plan(dec._h, vjp, 1, A["SDFR_DECODER_PLAN_TAPE"], steps, 64) == A["SDFR_E_INVALID"]
    assert L.sdfr_decoder_launch_plan(dec._h, fwd, 0, 0, steps, 64) == 0 and L.sdfr_decoder_launch_plan(dec._h, vjp, 0, 0, steps, 64) == 0
