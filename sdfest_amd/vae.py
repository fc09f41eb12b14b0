"""The SDF VAE: host-side mirror of ``sdfest/vae/sdf_vae.py`` -- SDFDecoder (:171-259), SDFEncoder (:103-169) and
SDFVAE (:11-101).

Built from the reference's own config dict (``decoder: {fc_layers, conv_layers}``,
``latent_size``, ``tsdf``) and a state dict with the reference's parameter names
(``decoder._fc_layers.{i}.weight`` ...).  ``forward`` / ``decode`` run in ``libsdfr_hip.so``
(decoder.hip): one launch for the Linear stack, one MFMA launch per Conv3d, one per resize.  The encoder runs in
encoder.hip (forward only): the layers whose activations do not fit in LDS one launch each, the rest with the heads
in one launch, one workgroup per sample.
"""
import ctypes
from typing import Mapping, Optional, Union

import numpy as np
import torch

from . import _lib
from .differentiable_renderer import _stream


def _flatten_state(state: Mapping, n_fc: int, n_conv: int, prefix: str) -> np.ndarray:
    def get(name):
        t = state[name]
        if isinstance(t, torch.Tensor):
            t = t.detach().cpu().numpy()
        return np.asarray(t, dtype=np.float32).reshape(-1)

    parts = []
    for i in range(n_fc):
        parts += [get(f"{prefix}_fc_layers.{i}.weight"), get(f"{prefix}_fc_layers.{i}.bias")]
    for i in range(n_conv):
        parts += [get(f"{prefix}_conv_layers.{i}.weight"), get(f"{prefix}_conv_layers.{i}.bias")]
    return np.ascontiguousarray(np.concatenate(parts))


class _DecodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, dec):
        zc = z.detach().contiguous()
        nbytes = dec._L.sdfr_decoder_tape_bytes(dec._h, zc.shape[0])
        tape = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dec.device)
        out = dec._forward_raw(zc, False, tape)
        ctx.save_for_backward(zc, tape)
        ctx.dec = dec
        return out

    @staticmethod
    def backward(ctx, grad_out):
        zc, tape = ctx.saved_tensors
        return ctx.dec._backward_raw(zc, tape, grad_out.contiguous()), None


class SDFDecoder:
    """Decoder of the SDF VAE (reference: SDFDecoder.__init__ sdf_vae.py:171-205)."""

    def __init__(self, volume_size: int, latent_size: int, fc_layers: list, conv_layers: list,
                 tsdf: Optional[Union[bool, float]] = False, state_dict: Optional[Mapping] = None,
                 device="cuda", prefix: str = "decoder."):
        # reference: SDFDecoder.sanity_check (sdf_vae.py:207-215)
        assert fc_layers[-1]["out"] == conv_layers[0]["in_channels"] * conv_layers[0]["in_size"] ** 3
        for a, b in zip(conv_layers[:-1], conv_layers[1:]):
            assert a["out_channels"] == b["in_channels"]
        assert conv_layers[-1]["out_channels"] == 1
        if state_dict is None:
            raise ValueError("state_dict with the decoder parameters is required")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._volume_size = volume_size
        self.latent_size = latent_size
        self._tsdf = tsdf
        if not any(k.startswith(prefix) for k in state_dict):
            prefix = ""
        params = _flatten_state(state_dict, len(fc_layers), len(conv_layers), prefix)
        arr = lambda v: np.ascontiguousarray(v, dtype=np.int32)
        fc_out = arr([l["out"] for l in fc_layers])
        ins = arr([l["in_size"] for l in conv_layers])
        cin = arr([l["in_channels"] for l in conv_layers])
        cout = arr([l["out_channels"] for l in conv_layers])
        ks = arr([l["kernel_size"] for l in conv_layers])
        relu = arr([1 if l["relu"] else 0 for l in conv_layers])
        L = _lib.lib()
        handle = ctypes.c_void_p()
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = L.sdfr_decoder_create(P(params), params.size, latent_size, len(fc_layers), P(fc_out),
                                   len(conv_layers), P(ins), P(cin), P(cout), P(ks), P(relu),
                                   volume_size, float(tsdf) if tsdf is not False else 0.0,
                                   self.device.index, ctypes.byref(handle))
        _lib.check(rc, "sdfr_decoder_create")
        self._L, self._h = L, handle
        self._ws = {}     # stream handle -> scratch buffer

    def narrow_linear_stack(self) -> bool:
        """Whether the Linear stack's leading layers run as ONE wave out of LDS (csrc/decoder_fc.hpp, fc_one_wave_ok: every
        layer input at most 64 wide, at most 8 layers, their parameters -- with the alignment gaps of the device image --
        within 6144 floats: the mug decoder's 8 -> 20 -> 50 -> 8192 does) and that form is switched on for this handle:
        what lets the captured loop's tail launch run the next iteration's Linear stack
        (``FusedRenderAndCompare(fc_in_tail=)``).  The library's own answer (``sdfr_decoder_fc_one_wave``): the criterion
        is stated once, on the C side, and the query changes nothing on the handle."""
        rc = self._L.sdfr_decoder_fc_one_wave(self._h)
        if rc < 0:
            _lib.check(rc, "sdfr_decoder_fc_one_wave")
        return rc == 1

    @classmethod
    def from_config(cls, config: Mapping, state_dict: Mapping, device="cuda", sdf_size: int = 64):
        """config: the reference's vae config (keys latent_size, decoder, tsdf)."""
        return cls(sdf_size, config["latent_size"], config["decoder"]["fc_layers"],
                   config["decoder"]["conv_layers"], config.get("tsdf", False), state_dict, device)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.sdfr_decoder_destroy(h)
            self._h = None

    OPTIONS = {name: _lib.ABI["SDFR_DECODER_OPT_" + name.upper()]      # include/sdfr.h
               for name in ("fused_resize", "tiled_vjp", "fc_one_wave", "fused_single")}

    def set_option(self, name: str, value: int) -> int:
        """Select one of two equivalent kernel forms for THIS decoder (``sdfr_decoder_set_option``: same results bit
        for bit, the defaults are the faster forms); returns the old value."""
        old = self._L.sdfr_decoder_set_option(self._h, self.OPTIONS[name], int(value))
        if old < 0:
            _lib.check(old, "sdfr_decoder_set_option")
        return old

    STEPS = {code: name[len("SDFR_DECODER_STEP_"):].lower()                  # include/sdfr.h
             for name, code in _lib.ABI.items() if name.startswith("SDFR_DECODER_STEP_")}

    def launch_plan(self, N: int, vjp: bool = False, tape: bool = False, stages: int = 3, enforce_tsdf: bool = False,
                    deferred: bool = False, scaled_views: int = 0) -> list:
        """The launches a forward (or, ``vjp=True``, a VJP) over N latents would make on this decoder, in order, as step
        names (``sdfr_decoder_launch_plan``: the planner the calls themselves launch from, asked for 256-byte aligned
        buffers; nothing is launched).  ``tape``, ``stages``, ``enforce_tsdf`` describe a forward; ``deferred`` and
        ``scaled_views`` (the scaled form's view count) a VJP."""
        A = _lib.ABI
        if vjp:
            flags = (A["SDFR_DECODER_PLAN_DEFERRED"] if deferred else 0) | (
                0 if not scaled_views else A["SDFR_DECODER_PLAN_SCALED_1"] if scaled_views == 1 else A["SDFR_DECODER_PLAN_SCALED_N"])
        else:
            flags = (A["SDFR_DECODER_PLAN_TAPE"] if tape else 0) | (A["SDFR_DECODER_PLAN_CLAMP"] if enforce_tsdf else 0) | {
                1: A["SDFR_DECODER_PLAN_STAGE_1"], 2: A["SDFR_DECODER_PLAN_STAGE_2"], 3: 0}[stages]
        steps = (ctypes.c_int * 128)()
        n = self._L.sdfr_decoder_launch_plan(self._h, A["SDFR_DECODER_PASS_VJP" if vjp else "SDFR_DECODER_PASS_FORWARD"],
                                             int(N), flags, steps, len(steps))
        if n < 0:
            _lib.check(n, "sdfr_decoder_launch_plan")
        return [self.STEPS[c] for c in steps[:n]]

    def _scratch(self, need: int) -> torch.Tensor:
        """Scratch of the calls on the CURRENT stream, grown on demand -- one buffer per stream, like the renderer's
        (``differentiable_renderer._workspace``): two streams driving the same decoder (the view generator decodes
        the next batch on a side stream while its consumer decodes or differentiates on its own) never share
        intermediate tensors without an ordering between them.  A buffer that is outgrown goes back to the caching
        allocator, which keeps it out of circulation until the work queued on ITS stream has finished."""
        key = _stream(self.device)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    def _forward_raw(self, zc: torch.Tensor, enforce_tsdf: bool, tape: Optional[torch.Tensor]):
        N, D = zc.shape[0], self._volume_size
        out = torch.empty((N, 1, D, D, D), dtype=torch.float32, device=self.device)
        ws = self._scratch(self._L.sdfr_decoder_workspace_bytes(self._h, N))
        rc = self._L.sdfr_decoder_forward(self._h, zc.data_ptr(), N, int(bool(enforce_tsdf)),
                                          out.data_ptr(), None if tape is None else tape.data_ptr(),
                                          ws.data_ptr(), ws.numel(),
                                          _stream(self.device))
        _lib.check(rc, "sdfr_decoder_forward")
        return out

    def _backward_raw(self, zc: torch.Tensor, tape: torch.Tensor, grad_out: torch.Tensor):
        N = zc.shape[0]
        g_z = torch.empty_like(zc)
        ws = self._scratch(self._L.sdfr_decoder_backward_workspace_bytes(self._h, N))
        rc = self._L.sdfr_decoder_backward_latent(self._h, zc.data_ptr(), tape.data_ptr(),
                                                  grad_out.data_ptr(), N, g_z.data_ptr(),
                                                  ws.data_ptr(), ws.numel(),
                                                  _stream(self.device))
        _lib.check(rc, "sdfr_decoder_backward_latent")
        return g_z

    def forward(self, z: torch.Tensor, enforce_tsdf: bool = False) -> torch.Tensor:
        """z (N, latent_size) -> (N, 1, D, D, D), like SDFDecoder.forward (sdf_vae.py:217-259).

        Differentiable w.r.t. z (the weights are constants, as in the estimation loop where only
        the latent is optimised, simple_setup.py:400-406)."""
        if not z.is_cuda or z.dtype != torch.float32:
            raise RuntimeError("z must be a float32 CUDA tensor")
        if z.dim() != 2 or z.shape[1] != self.latent_size:
            raise RuntimeError(f"z must have shape (N, {self.latent_size})")
        if z.requires_grad and torch.is_grad_enabled():
            if enforce_tsdf and self._tsdf is not False:
                raise NotImplementedError("gradient through the tsdf clamp is not supported")
            return _DecodeFn.apply(z, self)
        return self._forward_raw(z.detach().contiguous(), enforce_tsdf, None)

    __call__ = forward

    def decode(self, z: torch.Tensor, enforce_tsdf: bool = False) -> torch.Tensor:
        """Same as SDFVAE.decode (sdf_vae.py:79-87)."""
        return self.forward(z, enforce_tsdf)

    def jvp(self, z: torch.Tensor, tangents: Optional[torch.Tensor] = None, enforce_tsdf: bool = False):
        """The decoded volumes and their forward-mode derivative w.r.t. the latent (``sdfr_decoder_jvp``).

        z (N, latent_size); tangents (N, T, latent_size) directions per latent, None = the identity basis (T =
        latent_size: the full Jacobian d SDF / d z).  1 <= T <= SDFR_INFO_MAX_TANGENTS.  Returns ``(sdf, jac)``: sdf (N, 1, D, D, D) is the
        existing forward's output (run with a tape), jac the VOXEL-major buffer (N, D^3, Tp), Tp = T rounded up to a
        multiple of 4 with zeros in the columns T .. Tp - 1 -- ``jac[n, voxel, t]`` is the derivative of voxel `voxel`
        of latent n along ``tangents[n, t]``; this is the layout ``uncertainty.render_information(jacobian=)`` reads.
        ``SDFDecoder.tangent_volumes(jac, T)`` is the same memory as (N, T, D, D, D).  With ``enforce_tsdf`` on a
        truncating decoder the derivative is zero where the volume sits on the clamp.  No autograd: z is detached."""
        if not z.is_cuda or z.dtype != torch.float32:
            raise RuntimeError("z must be a float32 CUDA tensor")
        if z.dim() != 2 or z.shape[1] != self.latent_size:
            raise RuntimeError(f"z must have shape (N, {self.latent_size})")
        zc = z.detach().contiguous()
        N, D = zc.shape[0], self._volume_size
        if tangents is None:
            T, tc = self.latent_size, None
        else:
            if (not tangents.is_cuda or tangents.dtype != torch.float32 or tangents.dim() != 3
                    or tangents.shape[0] != N or tangents.shape[2] != self.latent_size):
                raise RuntimeError(f"tangents must be a float32 CUDA tensor of shape ({N}, T, {self.latent_size})")
            T, tc = tangents.shape[1], tangents.detach().contiguous()
        need = self._L.sdfr_decoder_jvp_workspace_bytes(self._h, N, T)
        if need == 0:
            raise RuntimeError(f"sdfr_decoder_jvp takes 1 <= T <= {_lib.ABI['SDFR_INFO_MAX_TANGENTS']} tangents and N T <= 65535 "
                               f"(N={N}, T={T})")
        tape = torch.empty(max(self._L.sdfr_decoder_tape_bytes(self._h, N) // 4, 1), dtype=torch.float32, device=self.device)
        out = self._forward_raw(zc, enforce_tsdf, tape)
        jac = torch.empty((N, D ** 3, (T + 3) & ~3), dtype=torch.float32, device=self.device)
        ws = self._scratch(need)
        clamp = bool(enforce_tsdf) and self._tsdf is not False
        rc = self._L.sdfr_decoder_jvp(self._h, zc.data_ptr(), tape.data_ptr(), out.data_ptr() if clamp else None,
                                      None if tc is None else tc.data_ptr(), N, T, int(clamp), jac.data_ptr(),
                                      ws.data_ptr(), ws.numel(), _stream(self.device))
        _lib.check(rc, "sdfr_decoder_jvp")
        return out, jac

    def decode_jvp(self, z: torch.Tensor, tangents: Optional[torch.Tensor] = None, enforce_tsdf: bool = False):
        """``jvp`` under the name ``SDFVAE.decode_jvp`` has (a pipeline holds either as its ``vae``)."""
        return self.jvp(z, tangents, enforce_tsdf)

    @staticmethod
    def tangent_volumes(jac: torch.Tensor, T: Optional[int] = None) -> torch.Tensor:
        """The (N, T, D, D, D) strided view of a ``jvp`` buffer (N, D^3, Tp): tangent volume t of latent n, no copy."""
        N, voxels, Tp = jac.shape
        D = round(voxels ** (1.0 / 3.0))
        if D ** 3 != voxels:
            raise RuntimeError("jac must be (N, D^3, Tp)")
        return jac.view(N, D, D, D, Tp)[..., :Tp if T is None else T].permute(0, 4, 1, 2, 3)


# ---- encoder ------------------------------------------------------------------------------------------------------
# reference: SDFEncoder (sdf_vae.py:103-169) builds `locate(type)(**args)` for every layer_infos entry; these are the
# types and arguments the kernels implement (encoder.hip).  Anything else is rejected when the encoder is created.
ENC_CONV, ENC_MAXPOOL, ENC_LINEAR, ENC_RELU = (_lib.ABI[f"SDFR_ENC_{t}"] for t in ("CONV", "MAXPOOL", "LINEAR", "RELU"))
_CONV_ARGS = {"in_channels", "out_channels", "kernel_size", "stride", "padding", "dilation", "groups", "bias",
              "padding_mode"}
_POOL_ARGS = {"kernel_size", "stride", "padding", "dilation", "return_indices", "ceil_mode"}


def _cubic(i, t, name, v):
    """an int, or a 3-sequence of one int (torch's _triple)"""
    if isinstance(v, (list, tuple)):
        if len(v) != 3 or len(set(v)) != 1:
            raise ValueError(f"layer {i} ({t}): {name}={v!r} is not cubic (only equal sizes along the three axes)")
        v = v[0]
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"layer {i} ({t}): {name}={v!r} is not supported (an int is required)")
    return int(v)


def _require(i, t, args, name, ok, default):
    if name in args and not ok(args[name]):
        raise ValueError(f"layer {i} ({t}): {name}={args[name]!r} is not supported (only {default!r})")


def parse_encoder_layers(volume_size: int, layer_infos: list) -> dict:
    """The reference's ``layer_infos`` -> the kernel's op list.

    Returns {"ops": [[type, a, b, kernel, stride, padding, relu, 0], ...] (the C ABI's rows), "params": the
    ``_features`` indices whose weight / bias the ops take, in order, "shapes": the activation shape after every layer
    ((C, S, S, S) or (F,)), "features": the heads' input size F}.  Raises ValueError naming the layer and the argument
    for anything the kernels do not implement; needs no GPU."""
    ops, params, shapes = [], [], []
    C, S, flat = 1, int(volume_size), False
    for i, info in enumerate(layer_infos):
        t = info.get("type")
        args = dict(info.get("args") or {})
        short = t.rsplit(".", 1)[-1] if isinstance(t, str) else None
        if not isinstance(t, str) or t not in (f"torch.nn.{short}", f"torch.nn.modules.{_MODULE.get(short)}.{short}") \
                or short not in ("Conv3d", "ReLU", "MaxPool3d", "Flatten", "Linear"):
            raise ValueError(f"layer {i}: type {t!r} is not supported (torch.nn.Conv3d, ReLU, MaxPool3d, Flatten, Linear)")
        if short == "Conv3d":
            unknown = set(args) - _CONV_ARGS
            if unknown:
                raise ValueError(f"layer {i} ({t}): argument {sorted(unknown)[0]!r} is not supported")
            for name in ("in_channels", "out_channels", "kernel_size"):
                if name not in args:
                    raise ValueError(f"layer {i} ({t}): {name} is required")
            if flat:
                raise ValueError(f"layer {i} ({t}): a Conv3d behind Flatten / Linear is not supported")
            cin, cout = _cubic(i, t, "in_channels", args["in_channels"]), _cubic(i, t, "out_channels", args["out_channels"])
            k = _cubic(i, t, "kernel_size", args["kernel_size"])
            s = _cubic(i, t, "stride", args.get("stride", 1))
            pad = args.get("padding", 0)
            p = 0 if pad == "valid" else _cubic(i, t, "padding", pad)
            if _cubic(i, t, "dilation", args.get("dilation", 1)) != 1:
                raise ValueError(f"layer {i} ({t}): dilation={args['dilation']!r} is not supported (only 1)")
            if _cubic(i, t, "groups", args.get("groups", 1)) != 1:
                raise ValueError(f"layer {i} ({t}): groups={args['groups']!r} is not supported (only 1)")
            _require(i, t, args, "bias", lambda v: v is True, True)
            _require(i, t, args, "padding_mode", lambda v: v == "zeros", "zeros")
            if cin != C:
                raise ValueError(f"layer {i} ({t}): in_channels={cin}, but its input has {C} channels")
            if cout < 1 or k < 1 or s < 1 or p < 0:
                raise ValueError(f"layer {i} ({t}): out_channels / kernel_size / stride / padding out of range")
            if S + 2 * p < k:
                raise ValueError(f"layer {i} ({t}): kernel_size={k} is larger than its padded input ({S + 2 * p})")
            C, S = cout, (S + 2 * p - k) // s + 1
            ops.append([ENC_CONV, cin, cout, k, s, p, 0, 0])
            params.append(i)
        elif short == "MaxPool3d":
            unknown = set(args) - _POOL_ARGS
            if unknown:
                raise ValueError(f"layer {i} ({t}): argument {sorted(unknown)[0]!r} is not supported")
            if "kernel_size" not in args:
                raise ValueError(f"layer {i} ({t}): kernel_size is required")
            if flat:
                raise ValueError(f"layer {i} ({t}): a MaxPool3d behind Flatten / Linear is not supported")
            k = _cubic(i, t, "kernel_size", args["kernel_size"])
            s = k if args.get("stride") is None else _cubic(i, t, "stride", args["stride"])
            if _cubic(i, t, "padding", args.get("padding", 0)) != 0:
                raise ValueError(f"layer {i} ({t}): padding={args['padding']!r} is not supported (only 0)")
            if _cubic(i, t, "dilation", args.get("dilation", 1)) != 1:
                raise ValueError(f"layer {i} ({t}): dilation={args['dilation']!r} is not supported (only 1)")
            _require(i, t, args, "return_indices", lambda v: v is False, False)
            _require(i, t, args, "ceil_mode", lambda v: v is False, False)
            if k < 1 or s < 1 or S < k:
                raise ValueError(f"layer {i} ({t}): kernel_size={k} / stride={s} do not fit its input ({S})")
            S = (S - k) // s + 1
            ops.append([ENC_MAXPOOL, 0, 0, k, s, 0, 0, 0])
        elif short == "Linear":
            unknown = set(args) - {"in_features", "out_features", "bias"}
            if unknown:
                raise ValueError(f"layer {i} ({t}): argument {sorted(unknown)[0]!r} is not supported")
            for name in ("in_features", "out_features"):
                if name not in args:
                    raise ValueError(f"layer {i} ({t}): {name} is required")
            _require(i, t, args, "bias", lambda v: v is True, True)
            if not flat:
                raise ValueError(f"layer {i} ({t}): Linear needs a flat input (a Flatten in front of it)")
            fin, fout = int(args["in_features"]), int(args["out_features"])
            if fin != C:
                raise ValueError(f"layer {i} ({t}): in_features={fin}, but its input has {C} features")
            if fout < 1:
                raise ValueError(f"layer {i} ({t}): out_features={fout}")
            C = fout
            ops.append([ENC_LINEAR, fin, fout, 0, 0, 0, 0, 0])
            params.append(i)
        elif short == "ReLU":
            unknown = set(args) - {"inplace"}
            if unknown:
                raise ValueError(f"layer {i} ({t}): argument {sorted(unknown)[0]!r} is not supported")
            if ops and ops[-1][0] != ENC_RELU:
                ops[-1][6] = 1                     # fused into the op in front of it (relu . relu = relu)
            elif not ops:
                ops.append([ENC_RELU, 0, 0, 0, 0, 0, 1, 0])
        else:  # Flatten: (C, D, H, W) is already the flat order
            _require(i, t, args, "start_dim", lambda v: v == 1, 1)
            _require(i, t, args, "end_dim", lambda v: v == -1, -1)
            unknown = set(args) - {"start_dim", "end_dim"}
            if unknown:
                raise ValueError(f"layer {i} ({t}): argument {sorted(unknown)[0]!r} is not supported")
            if not flat:
                C, flat = C * S ** 3, True
        shapes.append((C,) if flat else (C, S, S, S))
    if not flat:
        raise ValueError("the layers must end flat (a Flatten, as every reference config has): the heads take a vector")
    return {"ops": ops, "params": params, "shapes": shapes, "features": C}


_MODULE = {"Conv3d": "conv", "ReLU": "activation", "MaxPool3d": "pooling", "Flatten": "flatten", "Linear": "linear"}


def encoder_state_keys(plan: dict, prefix: str = "encoder.") -> list:
    """The reference's state-dict keys of an encoder, in the order the C ABI takes its parameters."""
    keys = []
    for i in plan["params"]:
        keys += [f"{prefix}_features.{i}.weight", f"{prefix}_features.{i}.bias"]
    for head in ("linear_means", "linear_log_var"):
        keys += [f"{prefix}{head}.weight", f"{prefix}{head}.bias"]
    return keys


def _encoder_params(plan: dict, latent: int, state: Mapping, prefix: str) -> np.ndarray:
    expect = []
    for op in plan["ops"]:
        if op[0] == ENC_CONV:
            expect += [(op[2], op[1], op[3], op[3], op[3]), (op[2],)]
        elif op[0] == ENC_LINEAR:
            expect += [(op[2], op[1]), (op[2],)]
    expect += [(latent, plan["features"]), (latent,)] * 2
    parts = []
    for key, shape in zip(encoder_state_keys(plan, prefix), expect):
        if key not in state:
            raise KeyError(f"state dict has no {key!r}")
        t = state[key]
        if isinstance(t, torch.Tensor):
            t = t.detach().cpu().numpy()
        t = np.asarray(t, dtype=np.float32)
        if t.shape != shape:
            raise ValueError(f"{key}: shape {t.shape}, the layers need {shape}")
        parts.append(t.reshape(-1))
    return np.ascontiguousarray(np.concatenate(parts))


def _check_grid(x: torch.Tensor, D: int, device: torch.device, what: str) -> None:
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError(f"{what} must be a float32 CUDA tensor")
    if x.dim() != 5 or x.shape[0] < 1 or tuple(x.shape[1:]) != (1, D, D, D):
        raise RuntimeError(f"{what} must have shape (N, 1, {D}, {D}, {D}) with N >= 1, got {tuple(x.shape)}")
    if x.device != device:
        raise RuntimeError(f"{what} is on {x.device}, the model on {device}")


def _seed(seed: Optional[int]) -> int:
    """seed=None: one draw from torch's default CPU generator (so torch.manual_seed makes runs repeatable)"""
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    return int(seed) & 0xFFFFFFFFFFFFFFFF


class SDFEncoder:
    """Encoder of the SDF VAE (reference: SDFEncoder, sdf_vae.py:103-169) on the GPU (csrc/encoder.hip).

    Forward only: there is no autograd through it (a call with ``x.requires_grad`` in grad mode raises)."""

    def __init__(self, volume_size: int, latent_size: int, layer_infos: list, tsdf: Optional[Union[bool, float]] = False,
                 state_dict: Optional[Mapping] = None, device="cuda", prefix: str = "encoder."):
        self.plan = parse_encoder_layers(volume_size, layer_infos)
        if state_dict is None:
            raise ValueError("state_dict with the encoder parameters is required")
        if not any(k.startswith(prefix) for k in state_dict):
            prefix = ""
        params = _encoder_params(self.plan, latent_size, state_dict, prefix)
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._volume_size = int(volume_size)
        self.latent_size = int(latent_size)
        self._tsdf = tsdf
        ops = np.ascontiguousarray(np.array(self.plan["ops"], dtype=np.int32).reshape(-1, _lib.ABI["SDFR_ENC_OP_INTS"]))
        L = _lib.lib()
        handle = ctypes.c_void_p()
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = L.sdfr_encoder_create(P(params), params.size, self._volume_size, self.latent_size, ops.shape[0], P(ops),
                                   self.device.index, ctypes.byref(handle))
        _lib.check(rc, "sdfr_encoder_create")
        self._L, self._h = L, handle
        self._ws = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.sdfr_encoder_destroy(h)
            self._h = None

    def _run(self, x: torch.Tensor, seed: Optional[int]):
        _check_grid(x, self._volume_size, self.device, "x")
        if x.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("the encoder has no autograd: call it under torch.no_grad() or on a tensor "
                                      "that does not require grad")
        xc = x.detach().contiguous()
        N, Ls = xc.shape[0], self.latent_size
        means = torch.empty((N, Ls), dtype=torch.float32, device=self.device)
        log_var = torch.empty_like(means)
        z = torch.empty_like(means) if seed is not None else None
        need = self._L.sdfr_encoder_workspace_bytes(self._h, N)
        key = _stream(self.device)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        rc = self._L.sdfr_encoder_forward(self._h, xc.data_ptr(), N, means.data_ptr(), log_var.data_ptr(),
                                          None if z is None else z.data_ptr(), 0 if seed is None else seed,
                                          ws.data_ptr(), ws.numel(), key)
        _lib.check(rc, "sdfr_encoder_forward")
        return means, log_var, z

    def forward(self, x: torch.Tensor):
        """x (N, 1, D, D, D) -> (means, log_var), each (N, latent_size)."""
        means, log_var, _ = self._run(x, None)
        return means, log_var

    __call__ = forward

    def prepare_input(self, sdfs: torch.Tensor) -> None:
        """Clamp to [-tsdf, tsdf] in place on the device when the model is truncated (sdf_vae.py:155-169)."""
        if self._tsdf is False:
            return
        if not isinstance(sdfs, torch.Tensor) or not sdfs.is_cuda or sdfs.dtype != torch.float32:
            raise RuntimeError("sdfs must be a float32 CUDA tensor")
        if not sdfs.is_contiguous():
            raise RuntimeError("sdfs must be contiguous (it is clamped in place)")
        with torch.no_grad():
            rc = self._L.sdfr_clamp(sdfs.data_ptr(), sdfs.numel(), float(self._tsdf), sdfs.device.index,
                                    _stream(sdfs.device))
        _lib.check(rc, "sdfr_clamp")


class SDFVAE:
    """The SDF VAE (reference: SDFVAE, sdf_vae.py:11-101): SDFEncoder + SDFDecoder on the GPU.

    Random numbers: ``encode`` / ``forward`` / ``sample`` / ``inference`` draw their noise from Philox-4x32-10 with
    Box-Muller (include/sdfr.h, group 7), not from ``torch.randn``: the values differ from the reference's, their
    distribution does not.  ``seed=None`` takes a seed from torch's default CPU generator, so ``torch.manual_seed``
    makes runs repeatable; row i of a batch depends on (seed, i) only."""

    def __init__(self, sdf_size: int, latent_size: int, encoder_dict: Mapping, decoder_dict: Mapping, device="cuda",
                 tsdf: Optional[Union[bool, float]] = False, state_dict: Optional[Mapping] = None):
        if state_dict is None:
            raise ValueError("state_dict with the VAE parameters is required")
        self.latent_size = latent_size
        self.sdf_size = sdf_size
        self._tsdf = tsdf
        self.encoder = SDFEncoder(sdf_size, latent_size, tsdf=tsdf, state_dict=state_dict, device=device,
                                  **encoder_dict)
        self.decoder = SDFDecoder(sdf_size, latent_size, tsdf=tsdf, state_dict=state_dict, device=device,
                                  **decoder_dict)
        self._device = self.encoder.device

    @classmethod
    def from_config(cls, config: Mapping, state_dict: Mapping, device="cuda", sdf_size: int = 64):
        """config: the reference's vae config (keys latent_size, encoder, decoder, tsdf)."""
        return cls(sdf_size, config["latent_size"], config["encoder"], config["decoder"], device,
                   config.get("tsdf", False), state_dict)

    def encode(self, x: torch.Tensor, seed: Optional[int] = None):
        """x (N, 1, D, D, D) -> (z, means, log_var); z = means + exp(0.5 log_var) eps (sdf_vae.py:65-71)."""
        means, log_var, z = self.encoder._run(x, _seed(seed))
        return z, means, log_var

    def forward(self, x: torch.Tensor, enforce_tsdf: bool = False, seed: Optional[int] = None):
        """-> (recon_x, means, log_var, z) (sdf_vae.py:53-58)."""
        z, means, log_var = self.encode(x, seed)
        return self.decoder(z, enforce_tsdf), means, log_var, z

    __call__ = forward

    def sample(self, n: int = 1, seed: Optional[int] = None) -> torch.Tensor:
        """(n, latent_size) standard normals: the encode noise with zero means and unit std (sdf_vae.py:60-63)."""
        if n < 0:
            raise ValueError("n must be >= 0")
        z = torch.empty((n, self.latent_size), dtype=torch.float32, device=self._device)
        rc = _lib.lib().sdfr_normal_sample(z.data_ptr(), n, self.latent_size, _seed(seed), self._device.index,
                                           _stream(self._device))
        _lib.check(rc, "sdfr_normal_sample")
        return z

    def inference(self, n: int = 1, enforce_tsdf: bool = False, seed: Optional[int] = None):
        """-> (recon_x, z) for n sampled latents (sdf_vae.py:73-77)."""
        z = self.sample(n, seed)
        return self.decoder(z, enforce_tsdf), z

    def decode(self, z: torch.Tensor, enforce_tsdf: bool = False) -> torch.Tensor:
        return self.decoder(z, enforce_tsdf)

    def decode_jvp(self, z: torch.Tensor, tangents: Optional[torch.Tensor] = None, enforce_tsdf: bool = False):
        """``SDFDecoder.jvp``: (sdf, jac) -- the decoded volumes and their derivative along latent directions."""
        return self.decoder.jvp(z, tangents, enforce_tsdf)

    def prepare_input(self, sdfs: torch.Tensor) -> None:
        self.encoder.prepare_input(sdfs)
