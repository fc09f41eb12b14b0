"""Single-shot initialisation network, inference only: host-side mirror of
``sdfest/initialization/pointnet.py::VanillaPointNet`` (:7-96),
``sdfest/initialization/sdf_pose_network.py::SDFPoseHead`` / ``SDFPoseNet`` (:9-147) and of
``SDFPipeline._nn_init`` (estimation/simple_setup.py:718-844), which runs it once before the
render-and-compare loop.  The arithmetic runs in ``libsdfr_hip.so`` (initnet.hip): per-point layers
as fp32 MFMA GEMMs with bias / BatchNorm / ReLU / residual / set-maximum epilogues, the head as
wave-per-row products, softmax + prior adjustment + argmax in one kernel.  ``features_batch`` / ``forward_batch`` run N
point sets per launch (initnet_eval.hip: the trainer's validation, sdfest_amd.init_train); row n has the bits of the
single-set call on set n.

Weights come as the state dict of the reference's ``SDFPoseNet`` (keys ``_backbone._linear_layers.i.*``,
``_backbone._bn_layers.i.*``, ``_head._linear_layers.i.*``, ``_head._bn_layers.i.*``,
``_head._final_layer.*``).  BatchNorm is applied in inference mode (running statistics), folded to a
scale and a shift per channel.  The trained weights of the paper are not in the reference repository
(download URLs only, mug.yaml:115-116); tests use seeded random weights of the mug architecture.
"""
from types import MappingProxyType
from typing import Dict, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._graphs import BoundedCache, capture
from .differentiable_renderer import Camera
from .pipeline import depth_to_pointcloud, quaternion_apply, quaternion_multiply
from .so3grid import SO3Grid

_BN_EPS = 1e-5  # torch.nn.BatchNorm1d default


class NoDepthError(Exception):
    """Raised when a depth image holds no valid pixel (simple_setup.py:30-32, :780-781)."""


def adjust_categorical_posterior(posterior: torch.Tensor, prior: torch.Tensor,
                                 train_prior: Optional[torch.Tensor]) -> torch.Tensor:
    """simple_setup.py:978-1009: posterior * prior / train_prior, L1-normalised along the last axis."""
    adjusted = posterior.clone() * prior
    if train_prior is not None:
        adjusted = adjusted / train_prior
    return torch.nn.functional.normalize(adjusted, p=1, dim=-1)


def _f32(t, dev):
    return torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).to(device=dev, dtype=torch.float32).contiguous()


def grid_quat_table(grid: SO3Grid, dev) -> torch.Tensor:
    """``SO3Grid.index_to_quat`` of every cell as a (C, 4) float32 device tensor"""
    return torch.tensor(np.stack([np.asarray(grid.index_to_quat(i), dtype=np.float64) for i in range(grid.num_cells())]),
                        dtype=torch.float32, device=dev).contiguous()


class _Layer:
    def __init__(self, state: Dict, prefix_lin: str, prefix_bn: Optional[str], dev):
        self.w = _f32(state[prefix_lin + ".weight"], dev)
        self.b = _f32(state[prefix_lin + ".bias"], dev)
        self.cout, self.cin_total = self.w.shape
        if prefix_bn is not None:
            g, beta = _f32(state[prefix_bn + ".weight"], dev), _f32(state[prefix_bn + ".bias"], dev)
            mu, var = _f32(state[prefix_bn + ".running_mean"], dev), _f32(state[prefix_bn + ".running_var"], dev)
            self.scale = (g / torch.sqrt(var + _BN_EPS)).contiguous()
            self.shift = (beta - mu * self.scale).contiguous()
        else:
            self.scale = torch.ones(self.cout, device=dev)
            self.shift = torch.zeros(self.cout, device=dev)


class SDFPoseNet:
    """``backbone`` / ``head``: the reference's config dictionaries (mug.yaml:98-111)."""

    def __init__(self, backbone: Dict, head: Dict, shape_dimension: int, state_dict: Dict, device="cuda"):
        self.dev = torch.device(device)
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.L = _lib.lib()
        self.in_size = int(backbone["in_size"])
        self.pn_sizes = list(backbone["mlp_out_sizes"])
        self.dense, self.residual = bool(backbone.get("dense", False)), bool(backbone.get("residual", False))
        bn_b = bool(backbone["batchnorm"])
        self.pn = [_Layer(state_dict, f"_backbone._linear_layers.{i}", f"_backbone._bn_layers.{i}" if bn_b else None,
                          self.dev) for i in range(len(self.pn_sizes))]
        bn_h = bool(head["batchnorm"])
        self.head = [_Layer(state_dict, f"_head._linear_layers.{i}", f"_head._bn_layers.{i}" if bn_h else None, self.dev)
                     for i in range(len(head["mlp_out_sizes"]))]
        self.final = _Layer(state_dict, "_head._final_layer", None, self.dev)
        self._backbone_plan = None                  # backbone_plan(), at its first call
        self.shape_dimension = int(shape_dimension)
        self.orientation_repr = head.get("orientation_repr", "quaternion")
        if self.orientation_repr == "discretized":
            self.grid = SO3Grid(head["orientation_grid_resolution"])
            n_out = self.shape_dimension + 4 + self.grid.num_cells()
        elif self.orientation_repr == "quaternion":
            self.grid, n_out = None, self.shape_dimension + 8
        else:
            raise NotImplementedError(f"orientation_repr {self.orientation_repr} is not supported.")
        if self.final.cout != n_out or self.head[0].cin_total != self.pn_sizes[-1]:
            raise RuntimeError("state dict does not match the head configuration")

    def _st(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def _vec(self, layer: _Layer, koff: int, x: Optional[torch.Tensor], k: int, bn: bool, relu: bool,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """act(bn(W[:, koff:koff + k] x + b)) of one vector (cout,), into `out` if given"""
        y = out if out is not None else torch.empty(layer.cout, dtype=torch.float32, device=self.dev)
        rc = self.L.sdfr_linear_vec(layer.w.data_ptr(), layer.cin_total, koff, x.data_ptr() if x is not None else None, k,
                                    layer.b.data_ptr(), layer.scale.data_ptr() if bn else None,
                                    layer.shift.data_ptr() if bn else None, int(relu), y.data_ptr(), layer.cout,
                                    self.dev.index, self._st())
        _lib.check(rc, "sdfr_linear_vec")
        return y

    def _rows(self, layer: _Layer, koff: int, x: torch.Tensor, k: int, bn: bool, relu: bool) -> torch.Tensor:
        """``_vec`` on the N rows of x (N, >= k): (N, cout) -- the same kernel, a row per ``blockIdx.y``"""
        N = x.shape[0]
        y = torch.empty((N, layer.cout), dtype=torch.float32, device=self.dev)
        rc = self.L.sdfr_linear_rows(layer.w.data_ptr(), layer.cin_total, koff, x.data_ptr(), x.shape[1], k,
                                     layer.b.data_ptr(), layer.scale.data_ptr() if bn else None,
                                     layer.shift.data_ptr() if bn else None, int(relu), y.data_ptr(), layer.cout,
                                     layer.cout, N, self.dev.index, self._st())
        _lib.check(rc, "sdfr_linear_rows")
        return y

    def backbone_plan(self) -> Tuple[Mapping, ...]:
        """What VanillaPointNet.forward (pointnet.py:61-96) decides per layer, decided once -- one record per layer:
        ``layer``; ``F_width`` / ``G_width``, the per-point and the broadcast part (a dense link's set maximum) of its
        input `prev_out`; ``out_width``, its output including a concatenated maximum; ``use_res``, a residual link
        (`prev_out.shape == out.shape`, :88-90); ``res_cat``, that residual is [F | G] concatenated (a dense link into
        a last layer as wide as both halves together), not F alone; ``last``.  Built at the first call (a state dict
        that does not match the configuration raises there), then the same read-only records every time."""
        if self._backbone_plan is None:
            plan = []
            F_width, G_width, prev_width, n = self.in_size, 0, self.in_size, len(self.pn)
            for i, layer in enumerate(self.pn):
                last = i == n - 1
                if layer.cin_total != F_width + G_width:
                    raise RuntimeError("state dict does not match the backbone configuration")
                out_width = layer.cout * (2 if (self.dense and not last) else 1)
                use_res = self.residual and prev_width == out_width
                plan.append(MappingProxyType(dict(
                    layer=layer, F_width=F_width, G_width=G_width, out_width=out_width, use_res=use_res,
                    res_cat=use_res and F_width != layer.cout, last=last)))
                G_width = layer.cout if (self.dense and not last) else 0
                F_width, prev_width = layer.cout, out_width
            self._backbone_plan = tuple(plan)
        return self._backbone_plan

    def _backbone(self, x: torch.Tensor, cnt: Optional[torch.Tensor], single: bool) -> torch.Tensor:
        """the backbone on the N sets x (N, M, in_size) -> (N, C_last).  single (N = 1, no counts): the single-set
        kernel, and torch pools a residual into the last layer; otherwise one batched launch per layer, whose kernel
        pools that residual itself (``pool_resid``)."""
        N, M = x.shape[0], x.shape[1]
        ptr = lambda t: t.data_ptr() if t is not None else None
        F, G = x, None       # the per-point part of `prev_out`, and its broadcast part (N, G_width): one row per set
        for p in self.backbone_plan():
            layer, F_width, last = p["layer"], p["F_width"], p["last"]
            # bias of the layer, plus the constant the concatenated maximum contributes to every point
            cvec = self._rows(layer, F_width, G, p["G_width"], False, False) if G is not None else layer.b
            pool = last and p["use_res"]
            colmax = torch.empty((N, layer.cout), dtype=torch.float32, device=self.dev)
            # the last layer stores nothing but its maxima, unless torch is to pool its residual sum
            store = not last or (pool and single)
            Y = torch.empty((N, M, layer.cout), dtype=torch.float32, device=self.dev) if store else None
            res_F = None
            if p["res_cat"]:
                res_F = torch.cat([F, G[:, None, :].expand(-1, M, -1)], dim=2).contiguous()
            elif p["use_res"]:
                res_F = F
            if single:
                rc = self.L.sdfr_pointnet_layer(F.data_ptr(), M, F_width, F.shape[2], layer.w.data_ptr(), layer.cin_total,
                                                cvec.data_ptr(), layer.scale.data_ptr(), layer.shift.data_ptr(),
                                                ptr(res_F), ptr(Y), layer.cout, layer.cout, colmax.data_ptr(),
                                                self.dev.index, self._st())
                _lib.check(rc, "sdfr_pointnet_layer")
            else:
                rc = self.L.sdfr_pointnet_layer_batch(
                    F.data_ptr(), ptr(cnt), N, M, F_width, F.shape[2], layer.w.data_ptr(), layer.cin_total,
                    cvec.data_ptr(), layer.cout if G is not None else 0, layer.scale.data_ptr(), layer.shift.data_ptr(),
                    ptr(res_F), ptr(Y), layer.cout, layer.cout, int(pool), colmax.data_ptr(), self.dev.index, self._st())
                _lib.check(rc, "sdfr_pointnet_layer_batch")
            if last:
                # torch.max over the points of the final `out` (after a residual, if any)
                return Y.max(dim=1).values if Y is not None else colmax
            # out = cat(out, max(out)); a residual adds prev_out = [F | G] to both halves
            G = (colmax + G if (p["use_res"] and G is not None) else colmax) if self.dense else None
            F = Y
        raise AssertionError

    def features(self, points: torch.Tensor) -> torch.Tensor:
        """VanillaPointNet.forward on ONE set (M, in_size) -> (C_last,) (pointnet.py:61-96)."""
        x = points.to(device=self.dev, dtype=torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] != self.in_size or x.shape[0] < 1:
            raise RuntimeError(f"points must have shape (M >= 1, {self.in_size})")
        return self._backbone(x[None], None, True)[0]

    def _split(self, out: torch.Tensor):
        """the head's output rows (N, L + 4 + C) or (N, L + 8) -> (latent (N,L), position (N,3), scale (N,), orientation:
        (N,C) logits, or the (N,4) quaternion normalised) (sdf_pose_network.py:93-115)"""
        sd = self.shape_dimension
        orientation = out[:, sd + 4:]
        if self.orientation_repr == "quaternion":
            orientation = orientation / torch.sqrt(torch.sum(orientation ** 2, 1, keepdim=True))
        return out[:, 0:sd], out[:, sd:sd + 3], out[:, sd + 3], orientation

    def head_forward(self, feature: torch.Tensor):
        """SDFPoseHead.forward on one feature vector (sdf_pose_network.py:70-115): (latent (1,L), position
        (1,3), scale (1,), orientation (1,4) normalised quaternion or (1,C) logits)."""
        out = feature
        for layer in self.head:
            out = self._vec(layer, 0, out, layer.cin_total, True, True)
        return self._split(self._vec(self.final, 0, out, self.final.cin_total, False, False)[None])

    def features_batch(self, points: torch.Tensor, counts=None) -> torch.Tensor:
        """VanillaPointNet.forward on N sets (N, M, in_size) -> (N, C_last): one launch per per-point layer, one
        ``sdfr_linear_rows`` per dense link, no synchronisation.  `counts` (int tensor or list, N entries): the real
        points of every set -- rows past counts[n] are ignored, a set without points gets a zero feature.  Row n equals
        ``features(points[n, :counts[n]])`` bit for bit."""
        x = points.to(device=self.dev, dtype=torch.float32).contiguous()
        if x.dim() != 3 or x.shape[2] != self.in_size or x.shape[0] < 1 or x.shape[1] < 1:
            raise RuntimeError(f"points must have shape (N >= 1, M >= 1, {self.in_size})")
        cnt = None
        if counts is not None:
            cnt = torch.as_tensor(counts).to(device=self.dev, dtype=torch.int32).contiguous()
            if cnt.shape != (x.shape[0],):
                raise RuntimeError(f"counts must have {x.shape[0]} entries")
        return self._backbone(x, cnt, False)

    def rows_batch(self, points: torch.Tensor, counts=None) -> torch.Tensor:
        """the head's output rows (N, L + 4 + C) or (N, L + 8) -- the quaternion before its normalisation -- of N sets:
        what ``sdfr_pose_metrics`` reads"""
        out = self.features_batch(points, counts)
        for layer in self.head:
            out = self._rows(layer, 0, out, layer.cin_total, True, True)
        return self._rows(self.final, 0, out, self.final.cin_total, False, False)

    def forward_batch(self, points: torch.Tensor, counts=None):
        """SDFPoseNet.forward on a batch (N, M, in_size): (latent (N,L), position (N,3), scale (N,), orientation (N,4)
        normalised quaternion or (N,C) logits)."""
        return self._split(self.rows_batch(points, counts))

    def grid_quats(self) -> Optional[torch.Tensor]:
        """the orientation of every cell (C, 4) on the device, built once; None for the quaternion head"""
        if self.grid is not None and getattr(self, "_grid_quats", None) is None:
            self._grid_quats = grid_quat_table(self.grid, self.dev)
        return self._grid_quats if self.grid is not None else None

    def __call__(self, points: torch.Tensor):
        """SDFPoseNet.forward: (N,M,3), or one point set as (1,M,3) or (M,3) (the estimator's use,
        simple_setup.py:786-787: the single-set kernels)."""
        if points.dim() == 3:
            if points.shape[0] != 1:
                return self.forward_batch(points)
            points = points[0]
        return self.head_forward(self.features(points))

    def orientation_posterior(self, logits: torch.Tensor, prior: Optional[torch.Tensor] = None,
                              train_prior: Optional[torch.Tensor] = None):
        """softmax, optional prior adjustment, argmax (simple_setup.py:795-812): (posterior (C,), index, max)."""
        lg = logits.reshape(-1).to(device=self.dev, dtype=torch.float32).contiguous()
        C = lg.numel()
        post = torch.empty(C, dtype=torch.float32, device=self.dev)
        idx = torch.empty(1, dtype=torch.int32, device=self.dev)
        mx = torch.empty(1, dtype=torch.float32, device=self.dev)
        pr = prior.reshape(-1).to(device=self.dev, dtype=torch.float32).contiguous() if prior is not None else None
        tp = (train_prior.reshape(-1).to(device=self.dev, dtype=torch.float32).contiguous()
              if (train_prior is not None and prior is not None) else None)
        rc = self.L.sdfr_orientation_posterior(lg.data_ptr(), C, pr.data_ptr() if pr is not None else None,
                                               tp.data_ptr() if tp is not None else None, post.data_ptr(),
                                               idx.data_ptr(), mx.data_ptr(), self.dev.index, self._st())
        _lib.check(rc, "sdfr_orientation_posterior")
        return post, idx, mx

    def orientation_topk(self, posterior: torch.Tensor, n: int):
        """the `n` most probable cells of a posterior (C,), descending; equal values by ascending index, a NaN below
        every number (``sdfr_orientation_topk``): (index (n,) int32, prob (n,)).  Entry 0 is ``orientation_posterior``'s
        index and maximum."""
        post = posterior.reshape(-1).to(device=self.dev, dtype=torch.float32).contiguous()
        n = int(n)
        idx = torch.empty(max(n, 0), dtype=torch.int32, device=self.dev)
        prob = torch.empty(max(n, 0), dtype=torch.float32, device=self.dev)
        rc = self.L.sdfr_orientation_topk(post.data_ptr(), post.numel(), n, idx.data_ptr(), prob.data_ptr(),
                                          self.dev.index, self._st())
        _lib.check(rc, "sdfr_orientation_topk")
        return idx, prob


def nn_init(network: SDFPoseNet, camera: Camera, depth_images: torch.Tensor, camera_positions: torch.Tensor,
            camera_orientations: torch.Tensor, config: Dict, normalize_pose: bool = True,
            prior_orientation_distribution: Optional[torch.Tensor] = None,
            training_orientation_distribution: Optional[torch.Tensor] = None):
    """``SDFPipeline._nn_init`` (simple_setup.py:718-844) for the VanillaPointNet backbone: per view
    depth -> point cloud (-> centroid removed) -> network -> estimate in the camera frame -> world frame;
    ``config["init_view"]`` "first" | "best" (largest posterior maximum, discretised orientations only);
    ``config["mean_shape"]`` zeroes the latent.  Returns (latent (1,L), position (1,3), scale (1,),
    orientation (1,4))."""
    if prior_orientation_distribution is not None and network.orientation_repr != "discretized":
        raise ValueError("prior_orientation_distribution only supported for discretized orientation representation.")
    best, best_result = 0, None
    for i, (depth_image, camera_orientation, camera_position) in enumerate(
            zip(depth_images, camera_orientations, camera_positions)):
        inp = depth_to_pointcloud(depth_image, camera)
        if len(inp) == 0:
            raise NoDepthError
        centroid = None
        if normalize_pose:
            centroid = torch.mean(inp, dim=-2)
            inp = inp - centroid
        latent_shape, position, scale, orientation_repr = network(inp.unsqueeze(0))
        if config.get("mean_shape", False):
            latent_shape = latent_shape.new_zeros(latent_shape.shape)
        if centroid is not None:
            position = position + centroid
        if network.orientation_repr == "discretized":
            prior = prior_orientation_distribution[i] if prior_orientation_distribution is not None else None
            _, index, maximum = network.orientation_posterior(orientation_repr, prior, training_orientation_distribution)
            orientation_camera = torch.tensor(network.grid.index_to_quat(int(index.item())), dtype=torch.float,
                                              device=network.dev).unsqueeze(0)
        else:
            orientation_camera, maximum = orientation_repr, None
        position_world = quaternion_apply(camera_orientation, position) + camera_position
        orientation_world = quaternion_multiply(camera_orientation, orientation_camera)
        strategy = config.get("init_view", "first")
        if strategy == "first":
            return latent_shape, position_world, scale, orientation_world
        elif strategy == "best":
            if network.orientation_repr != "discretized":
                raise NotImplementedError('"best" init strategy only supported with discretized '
                                          "orientation representation")
            if maximum.item() > best:
                best, best_result = maximum.item(), (latent_shape, position_world, scale, orientation_world)
        else:
            raise NotImplementedError('Only "first" and "best" strategies are currently supported')
    return best_result


class ResidentInit:
    """``SDFPipeline._nn_init`` (simple_setup.py:718-844) as a FIXED launch sequence with nothing read back: the number
    of observed points stays on the device (``sdfr_depth_count_centroid`` leaves count and centroid, the per-point
    layers are ``sdfr_pointnet_layer_counted``), the orientation cell's quaternion comes from a table uploaded once
    (``SO3Grid.index_to_quat`` of every cell), the camera -> world transform and the "first" / "best" choice are one
    small kernel (``sdfr_init_estimate``) that writes the estimate where the loop reads its parameters.  Every buffer
    is allocated at construction (points and activations at capacity, W * H rows), so the sequence can be captured
    into a hipGraph (``use_graph``) and the front door's call has no host synchronisation between the observation
    and the result.

    ``nn_init`` above stays the host-driven form (one call of ~25 launches, two host reads): same layers, same
    arithmetic per point; the centroid here is the count pass's fixed-order block-sum tree instead of ``torch.mean``
    (a few 1e-7 relative apart), so the two agree to rounding, not to the bit (tests/test_init_network_gpu.py).
    The empty-cloud check of :780-781 cannot raise before the launches it would prevent: ``empty_views()`` reads the
    counts afterwards (one small copy; the caller raises ``NoDepthError``)."""

    def __init__(self, network: SDFPoseNet, camera: Camera, views: int, config: Dict, normalize_pose: bool = True,
                 objects: bool = False, hypotheses: int = 1):
        """objects: the `views` images are `views` different OBJECTS seen from one camera (cam_pos / cam_quat hold one
        row): every image gets its own estimate, ``self.params`` is (views, 8 + L) -- the initialisation of
        ``pipeline.MultiObjectRenderAndCompare``; the "first" / "best" choice among views does not apply.
        hypotheses=N > 1 (one view of one object, discretised head): behind the estimate the N most probable cells of
        ``self.posterior`` (``sdfr_orientation_topk`` -> ``self.hyp_index`` / ``self.hyp_prob``, on the device) become N
        rows ``self.params_h`` (N, 8 + L) that differ in their orientation only (``sdfr_init_hypotheses``); row 0 is
        ``self.params``.  Both launches are part of the captured sequence.  With 1 the sequence is the one without."""
        net = self.net = network
        self.hypotheses = int(hypotheses)
        if not 1 <= self.hypotheses <= _lib.ABI["SDFR_MAX_HYPOTHESES"]:
            raise ValueError(f"hypotheses must be in [1, {_lib.ABI['SDFR_MAX_HYPOTHESES']}], got {hypotheses}")
        if self.hypotheses > 1 and (objects or int(views) != 1 or net.orientation_repr != "discretized"):
            raise ValueError("hypotheses > 1 needs one view of one object (views=1, objects=False) and a discretized "
                             "orientation head: the hypotheses are cells of its posterior")
        self.cam, self.V = camera, int(views)
        self.objects = bool(objects)
        self.dev, self.L = net.dev, net.L            # (L: the loaded library, as in SDFPoseNet)
        self.normalize_pose = bool(normalize_pose)
        self.mean_shape = bool(config.get("mean_shape", False))
        self.strategy = config.get("init_view", "first")
        if self.strategy not in ("first", "best"):
            raise NotImplementedError('Only "first" and "best" strategies are currently supported')
        if self.strategy == "best" and net.orientation_repr != "discretized":
            raise NotImplementedError('"best" init strategy only supported with discretized orientation representation')
        if net.in_size != 3:
            raise NotImplementedError("the resident form feeds back-projected points (in_size = 3)")
        H, W = camera.height, camera.width
        self.H, self.W, M = H, W, H * W
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.plan = net.backbone_plan()
        for p in self.plan:
            if p["res_cat"]:
                raise NotImplementedError("a residual link over a concatenated dense input: use nn_init")
            if p["last"] and p["use_res"]:
                raise NotImplementedError("a residual link into the last backbone layer: use nn_init")
        # (so every layer but the last stores its output, and the last leaves only its maxima)
        width = max([p["layer"].cout for p in self.plan if not p["last"]] + [4])
        self.points = torch.zeros((M, 3), **f32)
        self.act = [torch.zeros((M, width), **f32) for _ in range(2)]       # ping-pong per-point activations
        self.colmax = [torch.zeros(p["layer"].cout, **f32) for p in self.plan]
        self.cvec = [torch.zeros(p["layer"].cout, **f32) for p in self.plan]
        self.G = [torch.zeros(p["layer"].cout, **f32) for p in self.plan]
        self.head_vec = [torch.zeros(l.cout, **f32) for l in net.head] + [torch.zeros(net.final.cout, **f32)]
        i32 = dict(dtype=torch.int32, device=self.dev)
        self.count = torch.zeros(1, **i32)
        self.offset1 = torch.zeros(1, **i32)
        self.counts_all = torch.zeros(self.V, **i32)
        self.centroid = torch.zeros(3, **f32)
        self.ws = torch.zeros(max(self.L.sdfr_depth_centroid_workspace_bytes(1, W, H), 256) + 16, dtype=torch.uint8,
                              device=self.dev)
        self.discretized = net.orientation_repr == "discretized"
        if self.discretized:
            C = net.grid.num_cells()
            self.C = C
            self.grid_quats = torch.tensor(np.stack([np.asarray(net.grid.index_to_quat(i), dtype=np.float64)
                                                     for i in range(C)]), **f32).contiguous()
            self.posterior = torch.zeros(C, **f32)
            self.prior = torch.zeros((self.V, C), **f32)
            self.train_prior = torch.zeros(C, **f32)
        self.index = torch.zeros(1, **i32)
        self.post_max = torch.zeros(1, **f32)
        self.best = torch.zeros(1, **f32)
        self.params = torch.zeros((self.V, 8 + net.shape_dimension) if self.objects else (8 + net.shape_dimension,), **f32)
        if self.hypotheses > 1:
            if self.hypotheses > self.C:
                raise ValueError(f"hypotheses={self.hypotheses} exceed the grid's {self.C} cells")
            self.hyp_index = torch.zeros(self.hypotheses, **i32)
            self.hyp_prob = torch.zeros(self.hypotheses, **f32)
            self.params_h = torch.zeros((self.hypotheses, 8 + net.shape_dimension), **f32)
        self._graphs = BoundedCache(4)      # (a caller that hands other tensors every call: re-capture, no hoard)
        self._host_counts = torch.zeros(self.V, dtype=torch.int32).pin_memory()
        self._counts_event = None

    def _sequence(self, depth: torch.Tensor, cam_pos: torch.Tensor, cam_quat: torch.Tensor, has_prior: bool,
                  has_train: bool):
        """the launches, on the current stream; depth (V,H,W) float32 contiguous on the device"""
        L, net, d = self.L, self.net, self.dev.index
        st = torch.cuda.current_stream(self.dev).cuda_stream     # (the one `net._vec` launches on)
        fx, fy, cx0, cy0, _ = self.cam.get_pinhole_camera_parameters(0.0)
        W, H, M = self.W, self.H, self.W * self.H
        ws = self.ws[(-self.ws.data_ptr()) % 16:]
        views = range(self.V) if (self.strategy == "best" or self.objects) else range(1)
        best = self.strategy == "best" and not self.objects
        if best:
            self.best.zero_()
        order = _lib.ABI["SDFR_POINT_ORDER_ROW_MAJOR"]
        for v in views:
            img = depth[v]
            _lib.check(L.sdfr_depth_count_centroid(img.data_ptr(), 1, W, H, order, 1.0 / fx, 1.0 / fy, cx0, cy0,
                                                   self.count.data_ptr(), self.offset1.data_ptr(), self.centroid.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), d, st), "sdfr_depth_count_centroid")
            _lib.check(L.sdfr_depth_to_points_shifted(img.data_ptr(), 1, W, H, order, 1.0 / fx, 1.0 / fy, cx0, cy0,
                                                      self.offset1.data_ptr(), ws.data_ptr(),
                                                      self.centroid.data_ptr() if self.normalize_pose else None, None,
                                                      self.points.data_ptr(), d, st), "sdfr_depth_to_points_shifted")
            self.counts_all[v:v + 1].copy_(self.count)
            F, ldF = self.points, 3
            G = None
            for i, p in enumerate(self.plan):
                layer = p["layer"]
                if G is not None:     # bias + what the concatenated set maximum contributes to every point
                    cvec = net._vec(layer, p["F_width"], G, p["G_width"], False, False, out=self.cvec[i])
                else:
                    cvec = layer.b
                Y = self.act[i % 2] if not p["last"] else None
                ldy = Y.shape[1] if Y is not None else layer.cout
                rc = L.sdfr_pointnet_layer_counted(
                    F.data_ptr(), self.count.data_ptr(), M, p["F_width"], ldF, layer.w.data_ptr(), layer.cin_total,
                    cvec.data_ptr(), layer.scale.data_ptr(), layer.shift.data_ptr(),
                    F.data_ptr() if p["use_res"] else None, Y.data_ptr() if Y is not None else None, ldy, layer.cout,
                    self.colmax[i].data_ptr(), d, st)
                _lib.check(rc, "sdfr_pointnet_layer_counted")
                if net.dense and not p["last"]:
                    if p["use_res"] and G is not None:
                        torch.add(self.colmax[i], G, out=self.G[i])
                        G = self.G[i]
                    else:
                        G = self.colmax[i]
                else:
                    G = None
                if not p["last"]:
                    F, ldF = Y, ldy
            out = self.colmax[-1]
            for j, layer in enumerate(net.head):
                out = net._vec(layer, 0, out, layer.cin_total, True, True, out=self.head_vec[j])
            head = net._vec(net.final, 0, out, net.final.cin_total, False, False, out=self.head_vec[-1])
            sd = net.shape_dimension
            if self.discretized:
                _lib.check(L.sdfr_orientation_posterior(
                    head.data_ptr() + 4 * (sd + 4), self.C, self.prior[v].data_ptr() if has_prior else None,
                    self.train_prior.data_ptr() if (has_prior and has_train) else None, self.posterior.data_ptr(),
                    self.index.data_ptr(), self.post_max.data_ptr(), d, st), "sdfr_orientation_posterior")
            _lib.check(L.sdfr_init_estimate(
                head.data_ptr(), sd, self.grid_quats.data_ptr() if self.discretized else None,
                self.index.data_ptr() if self.discretized else None,
                self.centroid.data_ptr() if self.normalize_pose else None,
                cam_pos[0 if self.objects else v].data_ptr(), cam_quat[0 if self.objects else v].data_ptr(),
                int(self.mean_shape), int(best), self.post_max.data_ptr(), self.best.data_ptr(),
                (self.params[v] if self.objects else self.params).data_ptr(), d, st), "sdfr_init_estimate")
        if self.hypotheses > 1:     # (one view: self.posterior and self.params are that view's)
            _lib.check(L.sdfr_orientation_topk(self.posterior.data_ptr(), self.C, self.hypotheses,
                                               self.hyp_index.data_ptr(), self.hyp_prob.data_ptr(), d, st),
                       "sdfr_orientation_topk")
            _lib.check(L.sdfr_init_hypotheses(self.params.data_ptr(), self.params.numel(), self.grid_quats.data_ptr(),
                                              self.C, self.hyp_index.data_ptr(), self.hypotheses,
                                              cam_quat[0].data_ptr(), self.params_h.data_ptr(), d, st),
                       "sdfr_init_hypotheses")

    def __call__(self, depth: torch.Tensor, cam_pos: torch.Tensor, cam_quat: torch.Tensor,
                 prior_orientation_distribution: Optional[torch.Tensor] = None,
                 training_orientation_distribution: Optional[torch.Tensor] = None, use_graph: bool = True):
        """depth (V,H,W), cam_pos (V,3), cam_quat (V,4): float32, contiguous, on the device, and THE SAME TENSORS on
        every call when ``use_graph`` (their addresses are part of the captured sequence: the loop's target and camera
        buffers are such tensors).  Returns (latent (1,L), position (1,3), scale (1,), orientation (1,4)) as views of
        ``self.params``."""
        if prior_orientation_distribution is not None and not self.discretized:
            raise ValueError("prior_orientation_distribution only supported for discretized orientation representation.")
        has_prior = prior_orientation_distribution is not None
        has_train = has_prior and training_orientation_distribution is not None
        if has_prior:
            self.prior.copy_(prior_orientation_distribution.reshape(self.V, self.C))
        if has_train:
            self.train_prior.copy_(training_orientation_distribution.reshape(self.C))
        def sequence():
            self._sequence(depth, cam_pos, cam_quat, has_prior, has_train)

        if use_graph:
            key = (depth.data_ptr(), cam_pos.data_ptr(), cam_quat.data_ptr(), has_prior, has_train)
            # (warmed up on a side stream -- lazy module loads --, then captured; the sequence keeps no state between calls)
            self._graphs.get_or_build(key, lambda: capture(self.dev, (sequence,), sequence)[0]).replay()
        else:
            sequence()
        # the counts for the empty-cloud check, without waiting for them here
        self._host_counts.copy_(self.counts_all, non_blocking=True)
        self._counts_event = torch.cuda.Event()
        self._counts_event.record(torch.cuda.current_stream(self.dev))
        sd = self.net.shape_dimension
        p = self.params
        if self.objects:
            return p[:, 8:8 + sd], p[:, 0:3], p[:, 7], p[:, 3:7]
        return p[8:8 + sd][None], p[0:3][None], p[7:8], p[3:7][None]

    def empty_views(self):
        """the views (of those the strategy looked at) without a single observed point -- waits for the counts of the
        last call only (they were copied behind its launches), not for whatever was enqueued after them"""
        if self._counts_event is None:
            return []
        self._counts_event.synchronize()
        n = self.V if (self.strategy == "best" or self.objects) else 1
        return [v for v in range(n) if int(self._host_counts[v]) == 0]
