"""CPU twin of sdfest_amd/csrc/vae_train.hip: one training iteration of the SDF VAE (sdfest/vae/scripts/train.py:195-287)
as a plain torch statement -- forward, loss, autograd, torch.optim.Adam -- in float64 (or any dtype), for any supported
config.  The layer sequences are those of ``encoder_twin.torch_encoder`` and ``test_decoder_gpu.torch_decoder``, written
over tensors that require grad (the two convert their weights from numpy, which cuts the graph);
tests/test_vae_train_cpu.py checks that the three agree.  Never reads the reference."""
import numpy as np
import torch
import torch.nn.functional as F

TERMS = ("l2_small", "l2_large", "l1_small", "l1_large", "kld", "total")
WEIGHTS = {"l2_small_weight": 1.0, "l2_large_weight": 0.5, "l1_small_weight": 0.25, "l1_large_weight": 0.125,
           "kld_weight": 1.0}    # every term live (tools/make_vae_train_goldens.py)


def forward(params, config, x, eps):
    """(means, log_var, z, recon) of SDFVAE.forward(x, enforce_tsdf=False) with `eps` in place of torch.randn"""
    h = x
    for i, info in enumerate(config["encoder"]["layer_infos"]):
        t, a = info["type"].rsplit(".", 1)[-1], info.get("args") or {}
        if t == "Conv3d":
            h = F.conv3d(h, params[f"encoder._features.{i}.weight"], params[f"encoder._features.{i}.bias"],
                         stride=a.get("stride", 1), padding=a.get("padding", 0))
        elif t == "ReLU":
            h = torch.relu(h)
        elif t == "MaxPool3d":
            h = F.max_pool3d(h, a["kernel_size"], a.get("stride"))
        elif t == "Flatten":
            h = h.flatten(1)
        elif t == "Linear":
            h = F.linear(h, params[f"encoder._features.{i}.weight"], params[f"encoder._features.{i}.bias"])
        else:
            raise ValueError(t)
    means = F.linear(h, params["encoder.linear_means.weight"], params["encoder.linear_means.bias"])
    log_var = F.linear(h, params["encoder.linear_log_var.weight"], params["encoder.linear_log_var.bias"])
    z = eps * torch.exp(0.5 * log_var) + means
    fc, conv = config["decoder"]["fc_layers"], config["decoder"]["conv_layers"]
    out = z
    for i in range(len(fc)):
        out = F.relu(F.linear(out, params[f"decoder._fc_layers.{i}.weight"], params[f"decoder._fc_layers.{i}.bias"]))
    out = out.view(-1, conv[0]["in_channels"], *([conv[0]["in_size"]] * 3))
    for i, l in enumerate(conv):
        if out.shape[2] != l["in_size"]:
            out = F.interpolate(out, size=(l["in_size"],) * 3, mode="trilinear", align_corners=False)
        out = F.conv3d(out, params[f"decoder._conv_layers.{i}.weight"], params[f"decoder._conv_layers.{i}.bias"])
        if l["relu"]:
            out = F.relu(out)
    volume = int(config.get("sdf_size", 64))
    if out.shape[2] != volume:
        out = F.interpolate(out, size=(volume,) * 3, mode="trilinear", align_corners=False)
    return means, log_var, z, out


def loss(recon, x, means, log_var, config, post):
    """the six numbers of train.py:208-229, :271-281 (pc term left out) as a dict of tensors"""
    tsdf = config.get("tsdf", False)
    if tsdf is not False and post:
        mask = torch.logical_and(torch.abs(x) >= tsdf, torch.abs(recon) >= tsdf)
        temp = recon
        recon = temp.clone()
        recon[mask] = temp[mask].clamp(-tsdf, tsdf)
    l1 = torch.abs(recon - x)
    l2 = l1 ** 2
    small = torch.abs(x) < 0.1
    t = {"l2_small": torch.sum(l2[small]), "l2_large": torch.sum(l2[~small]), "l1_small": torch.sum(l1[small]),
         "l1_large": torch.sum(l1[~small]), "kld": -0.5 * torch.sum(1 + log_var - means.pow(2) - log_var.exp())}
    t["total"] = (config["l2_small_weight"] * t["l2_small"] + config["l2_large_weight"] * t["l2_large"]
                  + config["l1_small_weight"] * t["l1_small"] + config["l1_large_weight"] * t["l1_large"]
                  + t["kld"] * (config["kld_weight"] if post else 0))
    return t


class Twin:
    """parameters in `dtype` on the CPU, torch.optim.Adam(lr = learning_rate) over all of them, the iteration counter"""

    def __init__(self, config, state, dtype=torch.float64):
        self.config, self.dtype, self.iteration = dict(config), dtype, 0
        self.config.setdefault("warm_up_iterations", 1000)
        self.params = {k: torch.tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v), dtype=dtype,
                                       requires_grad=True) for k, v in state.items()}
        self.optimizer = torch.optim.Adam(list(self.params.values()), lr=self.config.get("learning_rate", 1e-3))

    def run(self, x, eps, iteration=None):
        """-> (terms: dict of floats, grads: dict of numpy float64, (means, log_var, z, recon) as numpy)"""
        it = self.iteration if iteration is None else iteration
        post = it > self.config["warm_up_iterations"]
        x = torch.as_tensor(np.asarray(x), dtype=self.dtype).clone()
        if post and self.config.get("tsdf", False) is not False:
            x.clamp_(-self.config["tsdf"], self.config["tsdf"])          # prepare_input
        out = forward(self.params, self.config, x, torch.as_tensor(np.asarray(eps), dtype=self.dtype))
        terms = loss(out[3], x, out[0], out[1], self.config, post)
        self.optimizer.zero_grad()
        terms["total"].backward()
        grads = {k: (np.zeros(p.shape) if p.grad is None else p.grad.detach().double().numpy().copy())
                 for k, p in self.params.items()}
        return ({k: float(v.detach()) for k, v in terms.items()}, grads, tuple(o.detach().double().numpy() for o in out))

    def step(self, x, eps):
        terms, _, _ = self.run(x, eps)
        self.optimizer.step()
        self.iteration += 1
        return terms


def blobs_at(size, seeds):
    """the `blobs` test volumes resampled to size^3 (trilinear, as the decoder resizes): (len(seeds), 1, size^3) float32"""
    from sdfest_amd.synthetic import blobs_sdf
    v = torch.tensor(np.stack([blobs_sdf(s) for s in seeds])[:, None])
    if size != v.shape[2]:
        v = F.interpolate(v, size=(size,) * 3, mode="trilinear", align_corners=False)
    return v.numpy().astype(np.float32)


def random_state(config, seed):
    """seeded He-scaled weights and small biases for any supported config (keys and shapes from the trainer's own table)"""
    from sdfest_amd.train import parameter_shapes
    rng = np.random.default_rng(seed)
    state = {}
    for key, shape in parameter_shapes(config):
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        scale = np.sqrt(2.0 / fan_in) if len(shape) > 1 else 0.05
        state[key] = (rng.standard_normal(shape) * scale).astype(np.float32)
    return state


def conv(i, c, o, k, relu):
    return dict(in_size=i, in_channels=c, out_channels=o, kernel_size=k, relu=relu)


def layer(t, **args):
    return {"type": f"torch.nn.{t}", "args": args}


# the smallest architectures at which each path of the kernels can still go wrong (tests/test_vae_train_gpu.py)
T16 = {"sdf_size": 16, "latent_size": 3, "tsdf": 0.1, "learning_rate": 1e-3, **WEIGHTS,
       "encoder": {"layer_infos": [layer("Conv3d", in_channels=1, out_channels=3, kernel_size=3, stride=2), layer("ReLU"),
                                   layer("Conv3d", in_channels=3, out_channels=5, kernel_size=3, stride=1, padding=1),
                                   layer("ReLU"), layer("MaxPool3d", kernel_size=2), layer("Flatten"),
                                   layer("Linear", in_features=135, out_features=12), layer("ReLU")]},
       "decoder": {"fc_layers": [{"out": 10}, {"out": 128}],
                   "conv_layers": [conv(4, 2, 6, 3, True), conv(7, 6, 4, 1, True), conv(12, 4, 1, 3, False)]}}
T8 = {"sdf_size": 8, "latent_size": 2, "tsdf": False, "learning_rate": 1e-3, **WEIGHTS,
      "encoder": {"layer_infos": [layer("Conv3d", in_channels=1, out_channels=2, kernel_size=3, padding=1), layer("ReLU"),
                                  layer("MaxPool3d", kernel_size=2, stride=2), layer("Flatten")]},
      "decoder": {"fc_layers": [{"out": 2 * 5 ** 3}],
                  "conv_layers": [conv(5, 2, 3, 3, True), conv(10, 3, 1, 3, False)]}}   # 10 - 3 + 1 = 8: no final resize


def mug_setup():
    """(config, state) of the reference's trained mug VAE from the goldens (decoder_mug.npz, mug_decoder_weights.npz,
    encoder_mug.npz), with the golden's loss weights"""
    import os
    import encoder_twin
    from helpers import GOLDEN
    d = np.load(os.path.join(GOLDEN, "decoder_mug.npz"))
    w = np.load(os.path.join(GOLDEN, "mug_decoder_weights.npz"))
    g = np.load(os.path.join(GOLDEN, "encoder_mug.npz"))
    state = {k: g[k] for k in g.files if k.startswith("encoder.")}
    state.update({k: w[k] for k in w.files})
    config = {"sdf_size": 64, "latent_size": int(d["latent_size"]), "tsdf": 0.1, "learning_rate": 1e-3, **WEIGHTS,
              "encoder": encoder_twin.MUG_ENCODER,
              "decoder": {"fc_layers": [{"out": int(o)} for o in d["fc_out"]],
                          "conv_layers": [conv(int(a), int(b), int(c), int(k), bool(r)) for a, b, c, k, r in
                                          zip(d["conv_in_size"], d["conv_cin"], d["conv_cout"], d["conv_k"],
                                              d["conv_relu"])]}}
    return config, state
