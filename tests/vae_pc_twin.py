"""CPU twin of the VAE trainer's point cloud term (csrc/vae_train.hip: sdfr_vae_trainer_pc_term, _pc_orientations;
sdfest/vae/scripts/train.py:230-269, :278) in float64: the orientation draw, the lift of a depth image, the term and its
gradient w.r.t. the reconstruction by autograd with the masked tsdf clamp, and -- composed with tests/vae_train_twin.py --
the seven loss numbers and every parameter gradient of an iteration.  Never reads the reference.

The in-volume mask is the term's only discontinuity: ``values`` asserts that no lifted point has a canonical coordinate
within ``MARGIN`` of +-1, so a comparison against float32 arithmetic never has to exclude a point."""
import numpy as np
import torch

import vae_train_twin as tw
from encoder_twin import philox4x32_10

PC_STREAM = 0x56415043          # counter word 3 of the orientation draw (include/sdfr.h)
POSITION, SCALE, THRESHOLD = (0.0, 0.0, -5.0), 1.0, 0.01      # train.py:255-263
CAMERA = (640, 480, 320.0, 320.0, 320.0, 240.0)               # W, H, fx, fy, cx, cy at pixel centre 0.5 (train.py:155)
MARGIN = 1e-3
TERMS = tw.TERMS + ("pc",)


def iteration_seed(seed, iteration):
    """SDFVAETrainer._iteration_seed: the Philox key of an iteration, a function of (seed, iteration)"""
    return (int(seed) * 0x9E3779B97F4A7C15 + int(iteration) * 0xD1B54A32D192ED03 + 1) & 0xFFFFFFFFFFFFFFFF


def orientations(key, n):
    """quat [n][4] float32 (x, y, z, w), uniform on SO(3) as train.py:242-251: counter {i, 0, 0, PC_STREAM}, key = the
    iteration seed; u_k = (word k - 1 >> 8) 2^-24; the expression in fp64, rounded once"""
    ctr = np.zeros((n, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 3] = np.arange(n, dtype=np.uint32), PC_STREAM
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(ctr, (np.uint32(key & 0xFFFFFFFF), np.uint32(key >> 32)))
    u1, u2, u3 = ((w[:, k] >> 8).astype(np.float64) / 16777216.0 for k in range(3))
    a, b = np.sqrt(1.0 - u1), np.sqrt(u1)
    return np.stack([a * np.sin(2 * np.pi * u2), a * np.cos(2 * np.pi * u2), b * np.sin(2 * np.pi * u3),
                     b * np.cos(2 * np.pi * u3)], 1).astype(np.float32)


def lift(depth, fx, fy, cx, cy):
    """(M, 3) float64 points of the non-zero pixels of one image, row-major (pointset_utils.py:57-77, "opengl"); cx, cy
    are pixel-centre-0.5 intrinsics, the lift's own are cx - 0.5, cy - 0.5 with integer pixel indices"""
    depth = torch.as_tensor(np.asarray(depth), dtype=torch.float64)
    rows, cols = torch.nonzero(depth, as_tuple=True)
    z = depth[rows, cols]
    return torch.stack(((cols.double() - (cx - 0.5)) * z / fx, -(rows.double() - (cy - 0.5)) * z / fy, -z), 1)


def canonical(points, position, quat, scale):
    """o = R(q / |q|)^T (P - position) / scale: the points in the volume's [-1, 1]^3 frame"""
    q = torch.as_tensor(np.asarray(quat), dtype=torch.float64)
    x, y, z, w = (q / torch.linalg.norm(q)).tolist()
    rot = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                        [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                        [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)
    return (points - torch.tensor(position, dtype=torch.float64)) @ rot / scale


def values(points, position, quat, scale, sdf, check_margin=True):
    """train.py's pc_loss (:30-125): the trilinear value of `sdf` (D, D, D) at every point, 0 where the base cell
    floor((o + 1) (D - 1) / 2) leaves [0, D - 2]^3.  Differentiable w.r.t. `sdf`."""
    D = sdf.shape[0]
    o = canonical(points, position, quat, scale)
    if check_margin and o.numel():
        gap = float((o.abs() - 1.0).abs().min())
        assert gap > MARGIN, f"a point lies {gap:.2e} from the volume's boundary (needs > {MARGIN})"
    g = (o + 1.0) * (D - 1) * 0.5
    cell = torch.floor(g)
    outside = (cell.min(dim=1)[0] < 0) | (cell.max(dim=1)[0] > D - 2) if o.numel() else torch.zeros(0, dtype=torch.bool)
    cell = cell.clamp(0, D - 2)
    f = g - cell
    c = cell.long()
    flat = sdf.reshape(-1)
    value = torch.zeros(o.shape[0], dtype=sdf.dtype)
    for k in range(8):
        ix, iy, iz = (k >> 2) & 1, (k >> 1) & 1, k & 1
        wk = (f[:, 0] if ix else 1 - f[:, 0]) * (f[:, 1] if iy else 1 - f[:, 1]) * (f[:, 2] if iz else 1 - f[:, 2])
        value = value + wk * flat[((c[:, 0] + ix) * D + c[:, 1] + iy) * D + c[:, 2] + iz]
    return torch.where(outside, torch.zeros_like(value), value), outside


def masked_clamp(recon, x, tsdf):
    """train.py:208-218: recon clamped to +-tsdf where |x| >= tsdf and |recon| >= tsdf (clone and assign)"""
    mask = torch.logical_and(torch.abs(x) >= tsdf, torch.abs(recon) >= tsdf)
    out = recon.clone()
    out[mask] = recon[mask].clamp(-tsdf, tsdf)
    return out


def term(recon, x, depth, quats, intrinsics, tsdf=0.0, position=POSITION, scale=SCALE, check_margin=True):
    """loss_pc = sum over the samples and their points of v^2 (a tensor; differentiable w.r.t. recon).  recon, x: (N,
    D, D, D) float64 tensors; depth (N, H, W); quats (N, 4); intrinsics (fx, fy, cx, cy) at pixel centre 0.5; tsdf > 0:
    the masked clamp is live.  Also returns the number of points inside / outside the volume per sample."""
    fx, fy, cx, cy = intrinsics
    if tsdf:
        recon = masked_clamp(recon, x, tsdf)
    N = recon.shape[0]
    positions = np.broadcast_to(np.asarray(position, dtype=np.float64), (N, 3))     # one pose for all, or one a sample
    scales = np.broadcast_to(np.asarray(scale, dtype=np.float64), (N,))
    total, counts = torch.zeros((), dtype=torch.float64), []
    for b in range(N):
        pts = lift(depth[b], fx, fy, cx, cy)
        v, outside = values(pts, positions[b].tolist(), quats[b], float(scales[b]), recon[b], check_margin)
        total = total + torch.sum(v ** 2)
        counts.append((int((~outside).sum()), int(outside.sum())))
    return total, counts


def term_and_gradient(recon, x, depth, quats, intrinsics, pc_weight, tsdf=0.0, position=POSITION, scale=SCALE):
    """(loss_pc, d (pc_weight loss_pc) / d recon as (N, D, D, D) float64 numpy, counts) by autograd"""
    r = torch.tensor(np.asarray(recon), dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(np.asarray(x), dtype=torch.float64)
    total, counts = term(r, xt, depth, quats, intrinsics, tsdf, position, scale)
    (pc_weight * total).backward()
    grad = np.zeros(r.shape) if r.grad is None else r.grad.numpy().copy()
    return float(total.detach()), grad, counts


class Twin(tw.Twin):
    """vae_train_twin.Twin with the pc_weight term: ``run`` takes the orientations and the depth images of the targets
    (both inputs: the render is the renderer's business) and returns the seven numbers (``TERMS``) and every gradient"""

    def run(self, x, eps, iteration=None, quats=None, depth=None, intrinsics=None):
        it = self.iteration if iteration is None else iteration
        cfg = self.config
        post = it > cfg["warm_up_iterations"]
        live = post and cfg.get("tsdf", False) is not False
        x = torch.as_tensor(np.asarray(x), dtype=self.dtype).clone()
        if live:
            x.clamp_(-cfg["tsdf"], cfg["tsdf"])          # prepare_input
        out = tw.forward(self.params, cfg, x, torch.as_tensor(np.asarray(eps), dtype=self.dtype))
        terms = tw.loss(out[3], x, out[0], out[1], cfg, post)
        terms["pc"], _ = term(out[3][:, 0], x[:, 0], depth, quats, intrinsics, cfg["tsdf"] if live else 0.0)
        terms["total"] = terms["total"] + cfg["pc_weight"] * terms["pc"]
        self.optimizer.zero_grad()
        terms["total"].backward()
        grads = {k: (np.zeros(p.shape) if p.grad is None else p.grad.detach().double().numpy().copy())
                 for k, p in self.params.items()}
        return ({k: float(v.detach()) for k, v in terms.items()}, grads, tuple(o.detach().double().numpy() for o in out))


def sparse(depth):
    """a depth image stack as (flat indices int64, values): how the goldens store it"""
    d = np.asarray(depth)
    idx = np.flatnonzero(d)
    return idx.astype(np.int64), d.reshape(-1)[idx]


def dense(idx, val, shape, dtype=np.float32):
    d = np.zeros(int(np.prod(shape)), dtype=dtype)
    d[idx] = val
    return d.reshape(shape)
