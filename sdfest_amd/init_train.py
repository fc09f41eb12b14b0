"""Training of the single-shot initialisation network on the GPU: host-side mirror of
``sdfest/initialization/scripts/train.py`` (``Trainer.run`` :130-150, ``_compute_loss`` :211-287) for the
``VanillaPointNet`` backbone and the ``SDFPoseHead``.

``SDFPoseNetTrainer`` owns the master parameters, their gradient and Adam's two moments as flat fp32 device buffers in the
reference's ``parameters()`` order, the BatchNorm running statistics as a fifth, and runs one iteration -- forward under
``train()`` with a tape, the four-term loss, the gradient of every parameter, Adam -- in ``libsdfr_hip.so``
(csrc/initnet_train.hip, include/sdfr.h group 11).  The batches come from ``SDFVAEViewGenerator`` (``collate``, ``fit``);
the trained state loads into the inference network unchanged (``net()``, ``init_network.SDFPoseNet``,
``SDFPipeline(init_state_dict=...)``).

Validation (train.py:344-374, :439-481): ``validation_set`` draws a fixed set once, ``validate`` runs the current state
under eval() over it -- ``SDFPoseNet.forward_batch`` and ``sdfr_pose_metrics`` (csrc/initnet_eval.hip),
one host read per set -- and ``geodesic_distance`` is the per-iteration metric of the training batch.

What the reference's loop has and this one does not: the other backbones, the NOCS / Redwood datasets and their mixing,
wandb and the visualisations.
"""
import ctypes
from typing import Dict, List, Mapping, Optional

import numpy as np
import torch

from . import _lib
from .differentiable_renderer import _stream
from .init_network import SDFPoseNet, grid_quat_table
from .so3grid import SO3Grid

TERMS = ("latent", "position", "scale", "orientation", "total")
WEIGHTS = ("latent_weight", "position_weight", "scale_weight", "orientation_weight")
_DEFAULTS = {"iterations": 1000000, "batch_size": 32, "learning_rate": 1e-3}
_TARGETS = ("latent_shape", "position", "scale", "orientation")
RECORD = ("position", "scale", "geodesic", "nll", "count")      # the fp64 record of sdfr_pose_metrics


def check_config(config: Mapping) -> dict:
    """The training config with the defaults filled in and ``orientation_repr`` / ``orientation_grid_resolution`` copied
    into the head (train.py:64-69); raises for what is missing or not implemented."""
    cfg = dict(_DEFAULTS)
    cfg.update(config)
    for key, only in (("backbone_type", "VanillaPointNet"), ("head_type", "SDFPoseHead")):
        if cfg.get(key, only) != only:
            raise NotImplementedError(f"{key}={cfg[key]!r}: only {only} is implemented")
    for key in ("backbone", "head", "orientation_repr", "vae") + WEIGHTS:
        if key not in cfg:
            raise KeyError(key)
    if "latent_size" not in cfg["vae"]:
        raise KeyError("vae.latent_size")
    head = dict(cfg["head"], orientation_repr=cfg["orientation_repr"])
    if "orientation_grid_resolution" in cfg:
        head["orientation_grid_resolution"] = cfg["orientation_grid_resolution"]
    if head["orientation_repr"] == "discretized":
        if head.get("orientation_grid_resolution") is None:
            raise KeyError("orientation_grid_resolution")
    elif head["orientation_repr"] != "quaternion":
        raise NotImplementedError(f"orientation_repr {head['orientation_repr']} is not supported.")
    cfg["head"], cfg["backbone"] = head, dict(cfg["backbone"])
    if int(cfg["head"]["in_size"]) != int(cfg["backbone"]["mlp_out_sizes"][-1]):
        raise ValueError("head.in_size must be the backbone's last width")
    return cfg


def num_cells(config: Mapping) -> int:
    """orientation classes of a checked config: the grid's cells, or 0 for the quaternion representation"""
    head = config["head"]
    return SO3Grid(head["orientation_grid_resolution"]).num_cells() if head["orientation_repr"] == "discretized" else 0


def parameter_shapes(config: Mapping) -> list:
    """[(state-dict key, shape)] of the network a checked `config` describes, in the reference's ``parameters()`` order =
    the flat buffers' order; needs no GPU."""
    bb, hd = config["backbone"], config["head"]
    latent, cells = int(config["vae"]["latent_size"]), num_cells(config)
    out, width = [], int(bb["in_size"])
    for i, c in enumerate(bb["mlp_out_sizes"]):
        out += [(f"_backbone._linear_layers.{i}.weight", (int(c), width)), (f"_backbone._linear_layers.{i}.bias", (int(c),))]
        width = 2 * int(c) if bb.get("dense", False) else int(c)
    if bb["batchnorm"]:
        for i, c in enumerate(bb["mlp_out_sizes"]):
            out += [(f"_backbone._bn_layers.{i}.weight", (int(c),)), (f"_backbone._bn_layers.{i}.bias", (int(c),))]
    width = int(hd["in_size"])
    for i, c in enumerate(hd["mlp_out_sizes"]):
        out += [(f"_head._linear_layers.{i}.weight", (int(c), width)), (f"_head._linear_layers.{i}.bias", (int(c),))]
        width = int(c)
    if hd["batchnorm"]:
        for i, c in enumerate(hd["mlp_out_sizes"]):
            out += [(f"_head._bn_layers.{i}.weight", (int(c),)), (f"_head._bn_layers.{i}.bias", (int(c),))]
    n_out = latent + 4 + (cells if cells else 4)
    return out + [("_head._final_layer.weight", (n_out, width)), ("_head._final_layer.bias", (n_out,))]


def stat_shapes(config: Mapping) -> list:
    """[(BatchNorm prefix, channels)] in the statistics buffer's order: {running_mean, running_var} each"""
    out = []
    for part in ("backbone", "head"):
        if config[part]["batchnorm"]:
            out += [(f"_{part}._bn_layers.{i}", int(c)) for i, c in enumerate(config[part]["mlp_out_sizes"])]
    return out


def initial_state(config: Mapping, seed: int = 0) -> dict:
    """torch's default initialisation drawn on the host: Linear weight and bias U(-b, b), b = 1 / sqrt(fan_in);
    BatchNorm weight 1, bias 0, running mean 0, running variance 1, no batch tracked."""
    config = check_config(config)
    gen = torch.Generator().manual_seed(int(seed))
    state, bound = {}, 0.0
    for key, shape in parameter_shapes(config):
        if "_bn_layers" in key:
            state[key] = torch.ones(shape) if key.endswith("weight") else torch.zeros(shape)
            continue
        if len(shape) > 1:
            bound = 1.0 / float(np.sqrt(shape[1]))
        state[key] = (torch.rand(shape, generator=gen, dtype=torch.float64) * 2.0 - 1.0).mul_(bound).float()
    for prefix, c in stat_shapes(config):
        state[prefix + ".running_mean"] = torch.zeros(c)
        state[prefix + ".running_var"] = torch.ones(c)
        state[prefix + ".num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    return state


def write_checkpoint(path: str, checkpoint: Mapping) -> None:
    torch.save(dict(checkpoint), path)


def read_checkpoint(path: str) -> dict:
    ck = torch.load(path, map_location="cpu", weights_only=False)
    for key in ("params", "stats", "batches_tracked", "exp_avg", "exp_avg_sq", "adam_step", "iteration", "seed", "config",
                "keys"):
        if key not in ck:
            raise ValueError(f"{path}: not a checkpoint of the initialisation network's trainer (no {key!r})")
    return ck


def _tensor(v):
    return v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))


def _metrics_call(L, out: torch.Tensor, latent: int, cells: int, grid_quats, position, scale, quat, index,
                  record: torch.Tensor) -> None:
    dev, N = out.device, out.shape[0]
    f32 = lambda t, shape: _tensor(t).to(device=dev, dtype=torch.float32).reshape(shape).contiguous()
    position, scale, quat = f32(position, (N, 3)), f32(scale, (N,)), f32(quat, (N, 4))
    if index is not None:
        index = _tensor(index).to(device=dev, dtype=torch.int32).reshape(N).contiguous()
    if record.dtype != torch.float64 or record.numel() != len(RECORD) or record.device != dev or not record.is_contiguous():
        raise ValueError(f"record must be a contiguous float64 tensor of {len(RECORD)} elements on {dev}")
    ws = torch.empty(L.sdfr_pose_metrics_workspace_bytes(N) // 8, dtype=torch.float64, device=dev)
    rc = L.sdfr_pose_metrics(out.data_ptr(), N, out.shape[1], latent, cells,
                             grid_quats.data_ptr() if grid_quats is not None else None, position.data_ptr(),
                             scale.data_ptr(), quat.data_ptr(), index.data_ptr() if index is not None else None,
                             record.data_ptr(), ws.data_ptr(), ws.numel() * 8, dev.index, _stream(dev))
    _lib.check(rc, "sdfr_pose_metrics")


def pose_metrics(net: SDFPoseNet, points: torch.Tensor, targets: Mapping, record: Optional[torch.Tensor] = None):
    """``net.rows_batch(points)`` and ``sdfr_pose_metrics`` against `targets`: "position" (N, 3), "scale" (N,),
    "quaternion" (N, 4) (a quaternion head also takes it from "orientation") and, for a discretized head, "orientation"
    (N,) class indices (optional: without them no NLL).  Adds the batch to `record` (``RECORD``: four fp64 sums and the
    sample count, on the device; default a new zero record) and returns it; nothing is read back."""
    discretized = net.orientation_repr == "discretized"
    quat = targets["quaternion"] if "quaternion" in targets else (None if discretized else targets["orientation"])
    if quat is None:
        raise KeyError("quaternion")
    if record is None:
        record = torch.zeros(len(RECORD), dtype=torch.float64, device=net.dev)
    out = net.rows_batch(points)
    cells = net.grid.num_cells() if discretized else 0
    _metrics_call(net.L, out, net.shape_dimension, cells, net.grid_quats(), targets["position"], targets["scale"], quat,
                  targets.get("orientation") if discretized else None, record)
    return record


def validation_keys(name: str, discretized: bool) -> list:
    """the reference's names of the validation numbers (train.py:459-472), in ``RECORD``'s order"""
    keys = [f"{name} validation mean position error / m", f"{name} validation mean scale error / m",
            f"{name} validation mean geodesic_distance / rad"]
    return keys + ([f"{name} validation orientation mean NLL"] if discretized else [])


class SDFPoseNetTrainer:
    """One initialisation network and its Adam state on the GPU.  ``config``: the reference's keys (backbone_type,
    backbone, head_type, head, orientation_repr, orientation_grid_resolution, vae.latent_size, learning_rate, batch_size,
    iterations, latent_weight, position_weight, scale_weight, orientation_weight)."""

    def __init__(self, config: Mapping, state_dict: Optional[Mapping] = None, seed: int = 0, device="cuda"):
        self.config = check_config(config)       # raises before anything touches the GPU
        cfg = self.config
        self._shapes = parameter_shapes(cfg)
        self._stat_shapes = stat_shapes(cfg)
        self.seed, self.iteration = int(seed), 0
        self.latent_size, self.cells = int(cfg["vae"]["latent_size"]), num_cells(cfg)
        self.in_size = int(cfg["backbone"]["in_size"])
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        L = _lib.lib()
        arr = lambda v: np.ascontiguousarray(v, dtype=np.int32)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        bb, hd = cfg["backbone"], cfg["head"]
        handle = ctypes.c_void_p()
        bb_out, hd_out = arr(bb["mlp_out_sizes"]), arr(hd["mlp_out_sizes"])
        rc = L.sdfr_pose_trainer_create(self.in_size, len(bb_out), P(bb_out), int(bool(bb["batchnorm"])),
                                        int(bool(bb.get("dense", False))), int(bool(bb.get("residual", False))),
                                        len(hd_out), P(hd_out), int(bool(hd["batchnorm"])), self.latent_size, self.cells,
                                        self.device.index, ctypes.byref(handle))
        _lib.check(rc, "sdfr_pose_trainer_create")
        self._L, self._h = L, handle
        count, stats = L.sdfr_pose_trainer_param_count(handle), L.sdfr_pose_trainer_stat_count(handle)
        assert count == sum(int(np.prod(s)) for _, s in self._shapes), "parameter layout differs from the library's"
        assert stats == 2 * sum(c for _, c in self._stat_shapes), "statistics layout differs from the library's"
        self.n_out = L.sdfr_pose_trainer_output_size(handle)
        f32 = dict(dtype=torch.float32, device=self.device)
        self._params = torch.zeros(count, **f32)
        self._grads = torch.zeros(count, **f32)
        self._exp_avg = torch.zeros(count, **f32)
        self._exp_avg_sq = torch.zeros(count, **f32)
        self._stats = torch.zeros(max(stats, 1), **f32)
        self._tracked = 0        # num_batches_tracked: the same number in every BatchNorm
        self._step = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._terms = torch.zeros(5, **f32)
        self._batch = {}         # (N, M) -> the buffers of an iteration
        self._collate_gen = torch.Generator().manual_seed((self.seed * 1000003 + 17) & 0x7FFFFFFFFFFFFFFF)
        self.load_state_dict(initial_state(cfg, self.seed) if state_dict is None else state_dict)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.sdfr_pose_trainer_destroy(h)
            self._h = None

    # ---- parameters --------------------------------------------------------------------------------------------------
    def _views(self, flat: torch.Tensor) -> dict:
        out, off = {}, 0
        for key, shape in self._shapes:
            n = int(np.prod(shape))
            out[key] = flat[off:off + n].view(shape)
            off += n
        return out

    def _stat_views(self) -> dict:
        out, off = {}, 0
        for prefix, c in self._stat_shapes:
            out[prefix + ".running_mean"] = self._stats[off:off + c]
            out[prefix + ".running_var"] = self._stats[off + c:off + 2 * c]
            off += 2 * c
        return out

    def state_dict(self) -> dict:
        """the reference's ``SDFPoseNet.state_dict()``: its keys, its order, copies on the device"""
        params, stats = self._views(self._params), self._stat_views()
        out = {}
        for key, _ in self._shapes:
            out[key] = params[key].clone()
            if "_bn_layers" in key and key.endswith(".bias"):
                prefix = key[:-len(".bias")]
                out[prefix + ".running_mean"] = stats[prefix + ".running_mean"].clone()
                out[prefix + ".running_var"] = stats[prefix + ".running_var"].clone()
                out[prefix + ".num_batches_tracked"] = torch.tensor(self._tracked, dtype=torch.int64, device=self.device)
        return out

    def load_state_dict(self, state: Mapping) -> None:
        parts = []
        for key, shape in self._shapes:
            if key not in state:
                raise KeyError(f"state dict has no {key!r}")
            t = _tensor(state[key])
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{key}: shape {tuple(t.shape)}, the layers need {tuple(shape)}")
            parts.append(t.detach().to(torch.float32).reshape(-1).cpu())
        stats = []
        for prefix, c in self._stat_shapes:
            for name in ("running_mean", "running_var"):
                if f"{prefix}.{name}" not in state:
                    raise KeyError(f"state dict has no '{prefix}.{name}'")
                t = _tensor(state[f"{prefix}.{name}"]).detach().to(torch.float32).reshape(-1).cpu()
                if t.numel() != c:
                    raise ValueError(f"{prefix}.{name}: {t.numel()} elements, the layer has {c} channels")
                stats.append(t)
            self._tracked = int(_tensor(state.get(f"{prefix}.num_batches_tracked", 0)))
        self._params.copy_(torch.cat(parts))
        if stats:
            self._stats.copy_(torch.cat(stats))

    def net(self) -> SDFPoseNet:
        """an inference network of the current state"""
        net = SDFPoseNet(self.config["backbone"], self.config["head"], self.latent_size, self.state_dict(),
                         device=self.device)
        net._grid_quats = self._grid_quats()      # (the cells' table is built once per trainer, not per validate())
        return net

    # ---- checkpoints -------------------------------------------------------------------------------------------------
    def save_checkpoint(self, path: str) -> None:
        write_checkpoint(path, {"params": self._params.cpu(), "stats": self._stats.cpu(), "batches_tracked": self._tracked,
                                "exp_avg": self._exp_avg.cpu(), "exp_avg_sq": self._exp_avg_sq.cpu(),
                                "adam_step": int(self._step.item()), "iteration": self.iteration, "seed": self.seed,
                                "collate_generator": self._collate_gen.get_state(), "config": dict(self.config),
                                "keys": [k for k, _ in self._shapes]})

    def load_checkpoint(self, path: str) -> None:
        ck = read_checkpoint(path)
        if ck["keys"] != [k for k, _ in self._shapes] or ck["params"].numel() != self._params.numel() or \
                ck["stats"].numel() != self._stats.numel():
            raise ValueError(f"{path}: the checkpoint is of another network")
        self._params.copy_(ck["params"])
        self._stats.copy_(ck["stats"])
        self._exp_avg.copy_(ck["exp_avg"])
        self._exp_avg_sq.copy_(ck["exp_avg_sq"])
        self._step.fill_(int(ck["adam_step"]))
        self._tracked, self.iteration, self.seed = int(ck["batches_tracked"]), int(ck["iteration"]), int(ck["seed"])
        if "collate_generator" in ck:
            self._collate_gen.set_state(ck["collate_generator"])

    # ---- one iteration -----------------------------------------------------------------------------------------------
    def _buffers(self, N: int, M: int) -> dict:
        b = self._batch.get((N, M))
        if b is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            L, h = self._L, self._h
            tape = L.sdfr_pose_trainer_tape_bytes(h, N, M)
            ws = L.sdfr_pose_trainer_workspace_bytes(h, N, M)
            if tape == 0 or ws == 0:
                raise ValueError(f"N = {N}, M = {M}: the library takes 1 <= N <= 65535 and N M <= 2^30, N >= 2 with a "
                                 "BatchNorm in the head and N M >= 2 with one in the backbone")
            b = {"points": torch.empty((N, M, self.in_size), **f32), "out": torch.empty((N, self.n_out), **f32),
                 "g_out": torch.empty((N, self.n_out), **f32), "latent_shape": torch.empty((N, self.latent_size), **f32),
                 "position": torch.empty((N, 3), **f32), "scale": torch.empty((N,), **f32),
                 "index": torch.zeros((N,), dtype=torch.int32, device=self.device), "quat": torch.zeros((N, 4), **f32),
                 "tape": torch.empty(tape, dtype=torch.uint8, device=self.device),
                 "ws": torch.empty(ws, dtype=torch.uint8, device=self.device)}
            self._batch = {(N, M): b}     # one batch shape at a time
        return b

    def _forward_backward(self, points: torch.Tensor, targets: Mapping, update_stats: bool) -> dict:
        if points.dim() != 3 or points.shape[2] != self.in_size or points.shape[0] < 1 or points.shape[1] < 1:
            raise ValueError(f"points must have shape (N, M, {self.in_size}), got {tuple(points.shape)}")
        N, M = int(points.shape[0]), int(points.shape[1])
        for key in _TARGETS:
            if key not in targets:
                raise KeyError(key)
        b = self._buffers(N, M)
        with torch.no_grad():
            b["points"].copy_(points)
            for key, shape in (("latent_shape", (N, self.latent_size)), ("position", (N, 3)), ("scale", (N,))):
                t = _tensor(targets[key])
                if tuple(t.shape) != shape:
                    raise ValueError(f"targets[{key!r}] must have shape {shape}, got {tuple(t.shape)}")
                b[key].copy_(t)
            o = _tensor(targets["orientation"])
            if tuple(o.shape) != ((N,) if self.cells else (N, 4)):
                raise ValueError(f"targets['orientation'] must have shape {(N,) if self.cells else (N, 4)}, "
                                 f"got {tuple(o.shape)}")
            b["index" if self.cells else "quat"].copy_(o)
            b["has_quat"] = not self.cells or "quaternion" in targets
            if self.cells and "quaternion" in targets:        # (only the metric reads it: geodesic_distance)
                q = _tensor(targets["quaternion"])
                if tuple(q.shape) != (N, 4):
                    raise ValueError(f"targets['quaternion'] must have shape {(N, 4)}, got {tuple(q.shape)}")
                b["quat"].copy_(q)
        cfg, L, h, st = self.config, self._L, self._h, _stream(self.device)
        p = lambda name: b[name].data_ptr()
        rc = L.sdfr_pose_trainer_forward(h, self._params.data_ptr(), self._stats.data_ptr(), p("points"), N, M,
                                         int(update_stats), p("out"), p("tape"), b["tape"].numel(), p("ws"),
                                         b["ws"].numel(), st)
        _lib.check(rc, "sdfr_pose_trainer_forward")
        rc = L.sdfr_pose_trainer_loss(h, p("out"), p("latent_shape"), p("position"), p("scale"),
                                      p("index") if self.cells else None, None if self.cells else p("quat"), N,
                                      float(cfg["latent_weight"]), float(cfg["position_weight"]),
                                      float(cfg["scale_weight"]), float(cfg["orientation_weight"]),
                                      self._terms.data_ptr(), p("g_out"), p("ws"), b["ws"].numel(), st)
        _lib.check(rc, "sdfr_pose_trainer_loss")
        rc = L.sdfr_pose_trainer_backward(h, self._params.data_ptr(), p("points"), N, M, p("tape"), p("g_out"),
                                          self._grads.data_ptr(), p("ws"), b["ws"].numel(), st)
        _lib.check(rc, "sdfr_pose_trainer_backward")
        return b

    def loss_and_grad(self, points: torch.Tensor, targets: Mapping) -> dict:
        """Forward under train(), loss and backward without an update and without a change of the running statistics.
        `points` (N, M, in_size); `targets`: "latent_shape" (N, L), "position" (N, 3), "scale" (N,), "orientation"
        (N,) class indices or (N, 4) quaternions.  Returns the five loss numbers (``TERMS``) as floats, ``grads``:
        name -> view of the gradient buffer, and ``out``: a clone of the head's output rows (N, L + 4 + C) or
        (N, L + 8), the quaternion before its normalisation."""
        b = self._forward_backward(points, targets, False)
        out = dict(zip(TERMS, self._terms.tolist()))
        out["grads"] = self._views(self._grads)
        out["out"] = b["out"].clone()
        return out

    def step(self, points: torch.Tensor, targets: Mapping) -> torch.Tensor:
        """One iteration: forward (the running statistics move), loss, backward, Adam.  Returns the five loss numbers
        (``TERMS``) as a device tensor, without synchronising."""
        self._forward_backward(points, targets, True)
        rc = self._L.sdfr_adam_flat(self._params.data_ptr(), self._grads.data_ptr(), self._exp_avg.data_ptr(),
                                    self._exp_avg_sq.data_ptr(), self._step.data_ptr(), self._params.numel(),
                                    float(self.config["learning_rate"]), self.device.index, _stream(self.device))
        _lib.check(rc, "sdfr_adam_flat")
        self.iteration += 1
        if self._stat_shapes:
            self._tracked += 1
        return self._terms.clone()

    # ---- metrics -----------------------------------------------------------------------------------------------------
    def _grid_quats(self):
        if self.cells and getattr(self, "_quat_table", None) is None:
            self._quat_table = grid_quat_table(SO3Grid(self.config["head"]["orientation_grid_resolution"]), self.device)
        return self._quat_table if self.cells else None

    def geodesic_distance(self) -> torch.Tensor:
        """The reference's "metric geodesic distance" (train.py:344-374) of the last ``step`` / ``loss_and_grad``: the
        batch mean of 2 acos(|q . q*|) between the target quaternions and the predicted ones (the argmax cell's, or the
        head's normalised), from the train-mode output rows the forward left, as a device scalar (float64).  Computed
        only here; a discretized head needs ``targets["quaternion"]`` next to the class indices."""
        if not self._batch:
            raise RuntimeError("geodesic_distance() follows a step() or loss_and_grad()")
        b = next(iter(self._batch.values()))
        if not b.get("has_quat"):
            raise KeyError("quaternion")
        record = torch.zeros(len(RECORD), dtype=torch.float64, device=self.device)
        _metrics_call(self._L, b["out"], self.latent_size, self.cells, self._grid_quats(), b["position"], b["scale"],
                      b["quat"], None, record)
        return record[2] / record[4]

    def validation_set(self, generator, samples: int, max_points: int = 2500, seed: int = 0) -> list:
        """`samples` valid samples of `generator` (a ``SDFVAEViewGenerator``), drawn once and collated into batches of
        ``batch_size`` (the last may be smaller) by ``collate``'s subset rule under its own generator seeded with `seed`:
        [(points (N, M, 3), targets)], the targets with "quaternion".  The set is fixed, so the numbers of ``validate``
        at different iterations are comparable."""
        if int(samples) < 1:
            raise ValueError("a validation set needs at least one sample")
        pending = []
        while len(pending) < int(samples):
            pending += self._valid_samples(generator.generate())
        pending = pending[:int(samples)]
        gen, bs = torch.Generator().manual_seed(int(seed)), int(self.config["batch_size"])
        return [self._collate_samples(pending[i:i + bs], max_points, gen) for i in range(0, len(pending), bs)]

    def validate(self, batches, name: str = "") -> dict:
        """The reference's ``_compute_validation_metrics`` (train.py:439-481) over `batches` ([(points, targets)], as
        ``validation_set`` returns): the current parameters and running statistics under eval() (``net()``), every
        batch through ``pose_metrics`` into one device record, ONE host read at the end.  Returns the reference's keys
        (``validation_keys``): each sum over the sample count.  The training state is not touched."""
        net = self.net()
        record = torch.zeros(len(RECORD), dtype=torch.float64, device=self.device)
        for points, targets in batches:
            pose_metrics(net, points, targets, record)
        sums = record.tolist()
        if sums[4] < 1:
            raise ValueError("validate() needs at least one batch")
        return {key: sums[i] / sums[4] for i, key in enumerate(validation_keys(name, bool(self.cells)))}

    # ---- batches -----------------------------------------------------------------------------------------------------
    def _collate_samples(self, samples: List[Dict], max_points: int, generator: Optional[torch.Generator]):
        gen = self._collate_gen if generator is None else generator
        M = min(min(int(s["pointset"].shape[0]) for s in samples), int(max_points))
        if M < 1:
            raise ValueError("a sample without points cannot be collated")
        sets = []
        for s in samples:
            pick = torch.randperm(int(s["pointset"].shape[0]), generator=gen)[:M].to(s["pointset"].device)
            sets.append(s["pointset"][pick])
        targets = {k: torch.stack([s[k] for s in samples]) for k in _TARGETS}
        if all("quaternion" in s for s in samples):      # (what the metrics compare with: geodesic_distance, validate)
            targets["quaternion"] = torch.stack([s["quaternion"] for s in samples])
        return torch.stack(sets), targets

    @staticmethod
    def _valid_samples(batch: Mapping) -> List[Dict]:
        valid = batch["valid"].tolist()
        keys = _TARGETS + (("quaternion",) if "quaternion" in batch else ())
        return [dict({k: batch[k][b] for k in keys}, pointset=batch["pointset"][b], index=b)
                for b in range(len(valid)) if valid[b]]

    def collate(self, batch: Mapping, max_points: int = 2500, generator: Optional[torch.Generator] = None):
        """``dataset_utils.collate_samples`` for a ``SDFVAEViewGenerator.generate()`` dictionary: the valid samples, every
        point set reduced to M = min(the smallest set, `max_points`) points drawn without replacement (`generator`: a
        host ``torch.Generator``; default the trainer's own, seeded from its seed).  Returns (points (N, M, 3), targets:
        "latent_shape", "position", "scale", "orientation", and "index": the kept samples' places in the batch)."""
        samples = self._valid_samples(batch)
        if not samples:
            raise ValueError("the batch has no valid sample")
        points, targets = self._collate_samples(samples, max_points, generator)
        targets["index"] = torch.tensor([s["index"] for s in samples], device=points.device)
        return points, targets

    def fit(self, generator, iterations: Optional[int] = None, log_every: int = 100, callback=None,
            max_points: int = 2500, validation: Optional[Mapping] = None, validation_every: Optional[int] = None) -> int:
        """The reference's loop: batches of exactly ``batch_size`` valid samples of `generator` (a
        ``SDFVAEViewGenerator``; invalid samples are redrawn, what a ``generate()`` leaves over opens the next batch)
        until the iteration counter reaches `iterations` (default: the config's).  The loss terms are copied to the host
        every `log_every` iterations only and given to ``callback(iteration, terms: dict)`` (default: print).
        `validation` ({name: batches of ``validation_set``}) with `validation_every`: every that many iterations
        ``validate`` runs over each set and its numbers join the dictionary (on such an iteration the callback is called
        whether it is a logged one or not), and a logged iteration also carries "metric geodesic distance".  Returns
        the number of ``generate()`` calls."""
        total = int(self.config["iterations"]) if iterations is None else int(iterations)
        bs = int(self.config["batch_size"])
        validating = bool(validation) and bool(validation_every)
        pending, calls = [], 0
        while self.iteration < total:
            while len(pending) < bs:
                pending += self._valid_samples(generator.generate())
                calls += 1
            points, targets = self._collate_samples(pending[:bs], max_points, None)
            pending = pending[bs:]
            terms = self.step(points, targets)
            logged = bool(log_every) and self.iteration % log_every == 0
            validated = validating and self.iteration % int(validation_every) == 0
            if logged or validated:
                named = dict(zip(TERMS, terms.tolist())) if logged else {}
                if logged and validating:
                    named["metric geodesic distance"] = float(self.geodesic_distance())
                if validated:
                    for name, batches in validation.items():
                        named.update(self.validate(batches, name))
                if callback is not None:
                    callback(self.iteration, named)
                else:
                    print(f"iteration {self.iteration}: " + ", ".join(f"{k} {v:.6g}" for k, v in named.items()),
                          flush=True)
        return calls
