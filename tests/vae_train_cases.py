"""The architectures the VAE trainer's kernels (sdfest_amd/csrc/vae_train.hip) are walked over, for
tests/test_vae_train_cases_cpu.py (the cases are what they claim to be), tests/test_vae_train_edges_gpu.py (``EDGES``)
and tests/test_vae_train_fuzz_gpu.py (``case(seed)``).  Everything here runs on the CPU, in torch: weights from
``vae_train_twin.random_state``, volumes from ``vae_train_twin.blobs_at``, eps from ``encoder_twin.normal_eps``.

A case is kept only where a comparison against float64 means something (``conditions``): no parameter's float64
gradient is identically zero, no value lies within 1e-5 of a branch it decides (``branch_margin``), torch in fp32 on the
CPU stays within 1e-5 of each gradient tensor's float64 maximum, the tsdf clamp's mask and the |x| < 0.1 split both have
members on either side.  Never reads the reference."""
import collections
import contextlib
import functools

import numpy as np
import torch
import torch.nn.functional as F

import encoder_twin as et
import vae_train_twin as tw
from vae_train_twin import conv, layer

PHASES = {"warm": 0, "post": 1001}        # iteration counters on the two sides of warm_up_iterations = 1000
MARGIN = 1e-5                             # smallest accepted branch_margin
FLOOR = 1e-5                              # largest accepted fp32 floor, of each gradient tensor's float64 maximum
SUB_DRAWS = 20

# the weight gradient's tiling (vae_train.hip: kWgCo, kWgRows, kWgT, kWgChunks, kCombineSlices)
WG_CO, WG_ROWS, WG_T, WG_CHUNKS, COMBINE_SLICES = 32, 32, 128, 4, 16
WAVE_SWITCH = 128                         # linear data gradient: a wave per element from this many outputs on


def net(sdf_size, latent, N, tsdf, encoder, fc, convs):
    return {"sdf_size": sdf_size, "latent_size": latent, "batch_size": N, "tsdf": tsdf, "learning_rate": 1e-3, **tw.WEIGHTS,
            "encoder": {"layer_infos": encoder}, "decoder": {"fc_layers": [{"out": o} for o in fc], "conv_layers": convs}}


def C3(cin, cout, k, s=1, p=0):
    return layer("Conv3d", in_channels=cin, out_channels=cout, kernel_size=k, stride=s, padding=p)


def P(k, s):
    return layer("MaxPool3d", kernel_size=k, stride=s)


def LIN(fin, fout):
    return layer("Linear", in_features=fin, out_features=fout)


R, FL = layer("ReLU"), layer("Flatten")

# name -> (config, seed of the weights and of eps).  The seed is the first of 0, 1, ... at which ``conditions`` holds.
EDGES = {
    # pool k = 3, s = 2 behind a conv (its data gradient runs): one element is the first maximum of up to 8 windows, the
    # lower window bound has negative numerators (x = 0: (0 - 3 + 2) / 2), 8 -> 3 leaves index 7 to no window
    "pool_overlap": (net(8, 2, 2, False, [C3(1, 3, 3, 1, 1), R, P(3, 2), FL], [2 * 27],
                         [conv(3, 2, 3, 2, True), conv(10, 3, 1, 3, False)]), 0),
    # pool k = 2, s = 3: indices 2, 5 and the tail 8 of 9 are read by no window (gradient exactly 0); 9 is the smallest
    # side with two gaps and a tail
    "pool_gapped": (net(9, 3, 2, 0.1, [C3(1, 4, 3, 1, 1), R, P(2, 3), FL], [10, 2 * 64],
                        [conv(4, 2, 3, 3, True), conv(11, 3, 1, 3, False)]), 1),
    # a pool in front of the first conv (first_param_op = 1: no data gradient into the pool), then pool k = 1, s = 2
    # with a ReLU flag on the pool (Conv, MaxPool, ReLU: the conv itself has none)
    "pool_first_k1_relu": (net(12, 2, 3, False, [P(2, 2), C3(1, 5, 3), P(1, 2), R, FL], [5 * 8],
                               [conv(2, 5, 4, 1, True), conv(7, 4, 1, 2, False)]), 0),
    # the common encoder layer k = 4, s = 2, p = 1 twice (the second has a data gradient): even kernel, stride with
    # padding; 17 -> 8 -> 4, the odd side leaves the windows of the first layer short of the far padding
    "conv_k4_s2_p1": (net(17, 4, 2, 0.3, [C3(1, 8, 4, 2, 1), R, C3(8, 13, 4, 2, 1), R, FL], [40, 3 * 27],
                          [conv(3, 3, 5, 2, True), conv(9, 5, 1, 2, False)]), 3),
    # k = 5, s = 3, p = 2 on 20 (-> 7: ox * 3 != tx for two of three taps) and k = 2, s = 3 on 7 (-> 2: index 2 lies
    # between the windows, 5 and 6 behind them: positions no window reaches), both behind a conv
    "conv_k5_s3_gaps": (net(20, 3, 2, 0.1, [C3(1, 3, 3, 1, 1), R, C3(3, 5, 5, 3, 2), R, C3(5, 8, 2, 3), R, FL], [20, 3 * 27],
                            [conv(3, 3, 4, 1, True), conv(8, 4, 1, 3, False)]), 1),
    # weight gradient: cout = 33 and 40 (a partial second channel group), R = 135, 264, 40 (no multiples of 32), 4^3 = 64
    # positions (below one chunk) and 17^3 = 4913 (10 ranges, the last one of 305: two full chunks, a part, then the
    # break), N ranges = 2 and 20: either side of 16.  The wide layers carry no ReLU: 2 x 40 x 4913 pre-activations
    # would leave no branch margin
    "wgrad_wide": (net(17, 5, 2, 0.1, [C3(1, 4, 3, 2), R, FL, LIN(4 * 512, 16), R], [20, 5 * 216],
                       [conv(6, 5, 33, 3, True), conv(18, 33, 40, 2, False), conv(17, 40, 1, 1, False)]), 1),
    # weight gradient at N = 1: 2^3 = 8 positions (below one chunk), 7^3 = 343 (between a chunk and a range), one record
    # each: 15 of the 16 combine slices are empty; latent 1
    "wgrad_one_record": (net(8, 1, 1, False, [C3(1, 2, 3, 1, 1), R, P(2, 2), FL], [2 * 64],
                             [conv(4, 2, 6, 3, True), conv(8, 6, 4, 2, True), conv(10, 4, 1, 3, False)]), 1),
    # resize down between two layers (6 -> 4, behind a ReLU: the mask goes through it) and a final resize down (10 -> 8)
    "resize_down": (net(8, 3, 2, 0.1, [C3(1, 3, 3, 2, 1), R, FL], [2 * 512],
                        [conv(8, 2, 4, 3, True), conv(4, 4, 3, 2, True), conv(12, 3, 1, 3, False)]), 1),
    # a source of size 1 (1 -> 5: every output reads index 0 twice) and a ReLU'd last conv without a final resize
    # (9 - 2 + 1 = 8: the backward starts with train_mask_kernel)
    "resize_from_1_last_relu": (net(8, 2, 2, False, [C3(1, 3, 3, 2), R, FL], [6, 4],
                                    [conv(1, 4, 6, 1, True), conv(5, 6, 3, 3, True), conv(9, 3, 1, 2, True)]), 0),
    # a ReLU'd last conv with a final resize behind it (7 -> 12): the mask passes through train_resize_dgrad_kernel
    "last_relu_final_resize": (net(12, 2, 2, 0.1, [C3(1, 3, 3, 2), R, P(2, 2), FL], [3 * 27],
                                   [conv(3, 3, 4, 2, True), conv(8, 4, 1, 2, True)]), 0),
    # Linear widths 127, 128, 129 on both sides of the cout >= 128 switch, each with a data gradient (a conv is the first
    # parameter op); 127 -> 128 has no ReLU between (Linear -> Linear); fin = 127 and 129: the tail of wave_dot
    "linear_127_128_129": (net(8, 3, 3, 0.3, [C3(1, 2, 3, 2), R, FL, LIN(54, 127), LIN(127, 128), R, LIN(128, 129), R],
                               [129, 127, 2 * 27], [conv(3, 2, 3, 1, True), conv(10, 3, 1, 3, False)]), 0),
    # an encoder without parameters (Flatten only): the heads read x, the backward ends at the heads; latent 1
    "flatten_only": (net(8, 1, 2, 0.1, [FL], [12, 2 * 27], [conv(3, 2, 3, 2, True), conv(10, 3, 1, 3, False)]), 0),
    # ReLU as the first layer: the one stand-alone relu op parse_encoder_layers emits
    "relu_first": (net(9, 2, 2, False, [R, C3(1, 3, 3, 2), R, FL, LIN(3 * 64, 7)], [16, 2 * 27],
                       [conv(3, 2, 3, 2, True), conv(11, 3, 1, 3, False)]), 0),
}


# ---- the op list, as sdfr_vae_trainer_create builds it ----------------------------------------------------------------
def train_ops(config):
    """dicts {type, cin, cout, n, m, k, s, p, relu, enc, gin} in the trainer's order; gin: its data gradient is computed
    (every decoder op; an encoder op behind the first one with parameters)"""
    from sdfest_amd.vae import ENC_CONV, ENC_LINEAR, ENC_MAXPOOL, parse_encoder_layers
    plan = parse_encoder_layers(config["sdf_size"], config["encoder"]["layer_infos"])
    ops, C, S, flat = [], 1, config["sdf_size"], False
    for t, a, b, k, s, p, relu, _ in plan["ops"]:
        if t == ENC_CONV:
            m = (S + 2 * p - k) // s + 1
            ops.append(dict(type="conv", cin=a, cout=b, n=S, m=m, k=k, s=s, p=p))
            C, S = b, m
        elif t == ENC_MAXPOOL:
            m = (S - k) // s + 1
            ops.append(dict(type="pool", cin=C, cout=C, n=S, m=m, k=k, s=s, p=0))
            S = m
        elif t == ENC_LINEAR:
            ops.append(dict(type="linear", cin=a, cout=b))
            flat = True
        else:
            ops.append(dict(type="relu", cin=C, cout=C, n=S, m=S))
        ops[-1].update(relu=bool(relu), enc=True)
    params = [i for i, op in enumerate(ops) if op["type"] in ("conv", "linear")]
    for i, op in enumerate(ops):
        op["gin"] = bool(params) and i > params[0]
    assert plan["features"] == (ops[-1]["cout"] if flat else C * S ** 3)
    width = config["latent_size"]
    for l in config["decoder"]["fc_layers"]:
        ops.append(dict(type="linear", cin=width, cout=l["out"], relu=True, enc=False, gin=True))
        width = l["out"]
    convs = config["decoder"]["conv_layers"]
    size = convs[0]["in_size"]
    for l in convs:
        if size != l["in_size"]:
            ops.append(dict(type="resize", cin=l["in_channels"], cout=l["in_channels"], n=size, m=l["in_size"], relu=False,
                            enc=False, gin=True))
        size = l["in_size"] - l["kernel_size"] + 1
        ops.append(dict(type="conv", cin=l["in_channels"], cout=l["out_channels"], n=l["in_size"], m=size,
                        k=l["kernel_size"], s=1, p=0, relu=bool(l["relu"]), enc=False, gin=True))
    if size != config["sdf_size"]:
        ops.append(dict(type="resize", cin=1, cout=1, n=size, m=config["sdf_size"], relu=False, enc=False, gin=True,
                        final=True))
    return ops, plan["features"]


PATHS = (
    "pool k > s", "pool k < s", "pool k = 1", "pool tail no window covers",
    "conv s > 1 and p > 0", "conv even k", "conv k = 4, s = 2, p = 1", "conv k = 5, s = 3", "conv positions no window reaches",
    "conv s = 3",
    "wgrad cout > 32, partial group", "wgrad R % 32 != 0", "wgrad positions below one chunk",
    "wgrad positions between a chunk and a range", "wgrad several ranges, short last", "wgrad N ranges < 16",
    "wgrad N ranges > 16",
    "resize down", "final resize down", "resize from 1",
    "linear cout = 127", "linear cout = 128", "linear cout = 129", "linear fin % 64 != 0 beyond 64",
    "encoder without parameters", "pool first", "relu first", "linear -> linear", "relu on a pool",
    "last relu, final resize", "last relu, no final resize", "latent 1",
)


def paths(config, N):
    """which of PATHS the trainer takes on `config` at batch size N, from the op shapes alone"""
    ops, features = train_ops(config)
    enc = [op for op in ops if op["enc"]]
    took = set()

    def take(path, cond):
        if cond:
            took.add(path)

    for i, op in enumerate(ops):
        t = op["type"]
        if t == "pool" and op["gin"]:
            k, s = op["k"], op["s"]
            take("pool k > s", k > s)
            take("pool k < s", k < s)
            take("pool k = 1", k == 1)
            take("pool tail no window covers", (op["n"] - k) % s)
        if t == "pool" and op["relu"]:
            took.add("relu on a pool")
        if t == "conv":
            k, s, p, n, m = op["k"], op["s"], op["p"], op["n"], op["m"]
            if op["gin"]:
                take("conv s > 1 and p > 0", s > 1 and p > 0)
                take("conv even k", k % 2 == 0)
                take("conv k = 4, s = 2, p = 1", (k, s, p) == (4, 2, 1))
                take("conv k = 5, s = 3", (k, s) == (5, 3))
                take("conv s = 3", s == 3)
                reached = {o * s - p + a for o in range(m) for a in range(k)}
                take("conv positions no window reaches", set(range(n)) - reached)
            R_, mv = op["cin"] * k ** 3, m ** 3
            ranges = -(-mv // (WG_T * WG_CHUNKS))
            take("wgrad cout > 32, partial group", op["cout"] > WG_CO and op["cout"] % WG_CO)
            take("wgrad R % 32 != 0", R_ % WG_ROWS)
            take("wgrad positions below one chunk", mv < WG_T)
            take("wgrad positions between a chunk and a range", WG_T < mv < WG_T * WG_CHUNKS)
            take("wgrad several ranges, short last", ranges > 1 and mv % (WG_T * WG_CHUNKS))
            take("wgrad N ranges < 16", N * ranges < COMBINE_SLICES)
            take("wgrad N ranges > 16", N * ranges > COMBINE_SLICES)
        if t == "resize":
            if op["m"] < op["n"]:
                took.add("final resize down" if op.get("final") else "resize down")
            take("resize from 1", op["n"] == 1)
            if op.get("final") and ops[i - 1]["relu"]:
                took.add("last relu, final resize")
        if t == "linear":
            if op["gin"] and op["cout"] in (WAVE_SWITCH - 1, WAVE_SWITCH, WAVE_SWITCH + 1):
                took.add(f"linear cout = {op['cout']}")
            take("linear fin % 64 != 0 beyond 64", op["cin"] > 64 and op["cin"] % 64)
            if op["enc"] and not op["relu"] and i + 1 < len(enc) and enc[i + 1]["type"] == "linear":
                took.add("linear -> linear")
    if features > 64 and features % 64:
        took.add("linear fin % 64 != 0 beyond 64")
    if not any(op["type"] in ("conv", "linear") for op in enc):
        took.add("encoder without parameters")
    if enc and enc[0]["type"] == "pool" and any(op["type"] in ("conv", "linear") for op in enc):
        took.add("pool first")
    if enc and enc[0]["type"] == "relu":
        took.add("relu first")
    if ops[-1]["type"] == "conv" and ops[-1]["relu"]:
        took.add("last relu, no final resize")
    if config["latent_size"] == 1:
        took.add("latent 1")
    assert took <= set(PATHS)
    return took


# ---- the branches -----------------------------------------------------------------------------------------------------
def traced_forward(params, config, x, eps):
    """``vae_train_twin.forward`` (tests/test_vae_train_cases_cpu.py: the same bits) that also returns every ReLU's input
    and every pool's input with its (k, s)"""
    relus, pools = [], []

    def relu(h):
        relus.append(h)
        return torch.relu(h)

    h = x
    for i, info in enumerate(config["encoder"]["layer_infos"]):
        t, a = info["type"].rsplit(".", 1)[-1], info.get("args") or {}
        if t == "Conv3d":
            h = F.conv3d(h, params[f"encoder._features.{i}.weight"], params[f"encoder._features.{i}.bias"],
                         stride=a.get("stride", 1), padding=a.get("padding", 0))
        elif t == "ReLU":
            h = relu(h)
        elif t == "MaxPool3d":
            pools.append((h, a["kernel_size"], a.get("stride") or a["kernel_size"]))
            h = F.max_pool3d(h, a["kernel_size"], a.get("stride"))
        elif t == "Flatten":
            h = h.flatten(1)
        else:
            h = F.linear(h, params[f"encoder._features.{i}.weight"], params[f"encoder._features.{i}.bias"])
    means = F.linear(h, params["encoder.linear_means.weight"], params["encoder.linear_means.bias"])
    log_var = F.linear(h, params["encoder.linear_log_var.weight"], params["encoder.linear_log_var.bias"])
    z = eps * torch.exp(0.5 * log_var) + means
    fc, convs = config["decoder"]["fc_layers"], config["decoder"]["conv_layers"]
    out = z
    for i in range(len(fc)):
        out = relu(F.linear(out, params[f"decoder._fc_layers.{i}.weight"], params[f"decoder._fc_layers.{i}.bias"]))
    out = out.view(-1, convs[0]["in_channels"], *([convs[0]["in_size"]] * 3))
    for i, l in enumerate(convs):
        if out.shape[2] != l["in_size"]:
            out = F.interpolate(out, size=(l["in_size"],) * 3, mode="trilinear", align_corners=False)
        out = F.conv3d(out, params[f"decoder._conv_layers.{i}.weight"], params[f"decoder._conv_layers.{i}.bias"])
        if l["relu"]:
            out = relu(out)
    if out.shape[2] != config["sdf_size"]:
        out = F.interpolate(out, size=(config["sdf_size"],) * 3, mode="trilinear", align_corners=False)
    return (means, log_var, z, out), relus, pools


def _near(values, level, scale):
    """the smallest | |v| - level | over `values`, relative to `scale`"""
    return float((values.abs() - level).abs().min() / scale)


def branch_margin(config, state, x, eps):
    """float64: the smallest distance of any value from a branch it decides, relative to its tensor's largest magnitude,
    over both phases -- every non-zero ReLU input from 0; the gap between the two largest values of every pool window in
    which they differ (a window whose two largest are equal is a tie at exactly 0 behind a ReLU, or one and the same
    constant: both sides then take the first, by construction); |x| from 0.1; after the warm-up |x| and |recon| from tsdf.
    |x| is the caller's volume: the post phase's clamp to +-tsdf moves nothing across 0.1 (tsdf >= 0.1 here) and leaves
    what it cuts at exactly tsdf, which both sides class alike (>= tsdf, and not < 0.1)."""
    tsdf = config.get("tsdf", False)
    params = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in state.items()}
    x64 = torch.tensor(np.asarray(x), dtype=torch.float64)
    e64 = torch.tensor(np.asarray(eps), dtype=torch.float64)
    worst = _near(x64, 0.1, x64.abs().max())
    for post in (False, True) if tsdf is not False else (False,):
        xin = x64.clamp(-tsdf, tsdf) if post else x64
        with torch.no_grad():
            (_, _, _, recon), relus, pools = traced_forward(params, config, xin, e64)
        for pre in relus:
            live = pre[pre != 0]
            if live.numel():
                worst = min(worst, float(live.abs().min() / pre.abs().max()))
        for h, k, s in pools:
            if k > 1:
                win = h.unfold(2, k, s).unfold(3, k, s).unfold(4, k, s).reshape(-1, k ** 3)
                top = torch.topk(win, 2, dim=1).values
                gap = (top[:, 0] - top[:, 1])
                gap = gap[gap > 0]
                if gap.numel():
                    worst = min(worst, float(gap.min() / h.abs().max()))
        if post:
            worst = min(worst, _near(x64, tsdf, x64.abs().max()), _near(recon, tsdf, recon.abs().max()))
    return worst


# ---- the conditions ---------------------------------------------------------------------------------------------------
Report = collections.namedtuple("Report", "margin floor zero_gradients small_split clamp_split")
Case = collections.namedtuple("Case", "name seed sub config state x eps report reference")


@contextlib.contextmanager
def one_thread():
    """torch on one CPU thread for the twins: layers this small run a hundred times slower when every op is split
    over a pool of threads, and one thread gives the fp32 twin one summation order on every machine"""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(before)


def conditions(config, state, x, eps):
    """-> (Report, reference): reference[phase] = the float64 twin's (terms, grads, (means, log_var, z, recon)); the
    Report's fields are what ``accepted`` judges"""
    with one_thread():
        return _conditions(config, state, x, eps)


def _conditions(config, state, x, eps):
    reference, floor, zero = {}, 0.0, []
    for phase, it in PHASES.items():
        reference[phase] = tw.Twin(config, state).run(x, eps, it)
        _, g32, _ = tw.Twin(config, state, dtype=torch.float32).run(x, eps, it)
        for name, g64 in reference[phase][1].items():
            top = np.abs(g64).max()
            if top == 0:
                zero.append(f"{phase}: {name}")
            else:
                floor = max(floor, float(np.abs(g32[name] - g64).max() / top))
    small = np.abs(np.asarray(x)) < 0.1
    tsdf = config.get("tsdf", False)
    clamp_split = True
    if tsdf is not False:
        recon = reference["post"][2][3]
        mask = (np.abs(np.asarray(x, np.float64)) >= tsdf) & (np.abs(recon) >= tsdf)
        clamp_split = bool(mask.any() and not mask.all())
    report = Report(branch_margin(config, state, x, eps), floor, zero, bool(small.any() and not small.all()), clamp_split)
    return report, reference


def accepted(report):
    return (not report.zero_gradients and report.margin >= MARGIN and report.floor <= FLOOR and report.small_split
            and report.clamp_split)


@functools.lru_cache(maxsize=None)
def volumes(size, N):
    return tw.blobs_at(size, tuple(range(N)))


def setup(name, config, seed, sub=None):
    N, state = config["batch_size"], tw.random_state(config, seed if sub is None else 1000 * seed + sub)
    x, eps = volumes(config["sdf_size"], N), et.normal_eps(seed, N, config["latent_size"])
    report, reference = conditions(config, state, x, eps)
    return Case(name, seed, sub, config, state, x, eps, report, reference)


@functools.lru_cache(maxsize=None)
def edge(name):
    return setup(name, *EDGES[name])


# ---- the random walk --------------------------------------------------------------------------------------------------
CHANNELS = (1, 3, 5, 8, 13, 33, 40)
MACS = 2e7            # per layer and sample: keeps the two CPU twins of a case well below a second


def draw(seed, sub):
    """a seeded config; may be one ``parameter_shapes`` rejects or ``conditions`` do not hold for (``case`` goes on)"""
    rng = np.random.default_rng([0x7AE, seed, sub])
    pick = lambda values: values[int(rng.integers(len(values)))]
    D, L, N = pick((8, 9, 12, 16, 17, 20)), int(rng.integers(1, 9)), pick((1, 2, 3, 5))
    layers, C, S = [], 1, D

    def pool():
        nonlocal S
        k, s = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        if S >= k:
            layers.append(P(k, s))
            S = (S - k) // s + 1
            if rng.random() < 0.2:
                layers.append(R)

    if rng.random() < 0.1:
        layers.append(R)
    if rng.random() < 0.1:
        pool()
    for _ in range(int(rng.integers(0, 4))):
        k, s, p = int(rng.integers(1, 6)), int(rng.integers(1, 4)), int(rng.integers(0, 3))
        if S + 2 * p < k:
            continue
        m = (S + 2 * p - k) // s + 1
        fits = [c for c in CHANNELS if C * c * k ** 3 * m ** 3 <= MACS]
        cout = pick(fits)
        layers.append(C3(C, cout, k, s, p))
        C, S = cout, m
        if rng.random() < 0.7:
            layers.append(R)
        if rng.random() < 0.4:
            pool()
    layers.append(FL)
    width = C * S ** 3
    for _ in range(int(rng.integers(0, 3))):
        out = pick((1, 7, 64, 65, 130))
        if width * out <= 2e6:
            layers.append(LIN(width, out))
            width = out
            if rng.random() < 0.6:
                layers.append(R)
    fc = [pick((3, 20, 64, 70, 128, 200)) for _ in range(int(rng.integers(0, 3)))]
    n_conv = int(rng.integers(1, 4))
    convs, size, cin = [], None, None
    for l in range(n_conv):
        if l == 0:
            in_size = int(rng.integers(1, 7))
            cin = pick([c for c in CHANNELS if c * in_size ** 3 <= 4096])
        else:
            in_size = int(np.clip(size + rng.integers(-3, 9), 1, 20))
        k = int(rng.integers(1, min(4, in_size) + 1))
        while cin * k ** 3 > 960:      # the trainer's limit on a decoder layer's cin k^3
            k -= 1
        m = in_size - k + 1
        fits = [c for c in CHANNELS if cin * c * k ** 3 * m ** 3 <= MACS] or [1]
        cout = 1 if l == n_conv - 1 else pick(fits)
        relu = bool(rng.random() < (0.2 if l == n_conv - 1 else 0.8))
        convs.append(conv(in_size, cin, cout, k, relu))
        size, cin = m, cout
    fc.append(convs[0]["in_channels"] * convs[0]["in_size"] ** 3)
    return net(D, L, N, pick((False, 0.1, 0.3)), layers, fc, convs)


def describe(config):
    """the op list on one line, for assertion messages"""
    ops, _ = train_ops(config)
    words = []
    for op in ops:
        t = op["type"]
        if t in ("conv", "pool"):
            w = f"{t}({op['cin']}->{op['cout']} k{op['k']} s{op['s']} p{op['p']} {op['n']}->{op['m']})"
        elif t == "linear":
            w = f"linear({op['cin']}->{op['cout']})"
        else:
            w = f"{t}({op['cin']} {op['n']}->{op['m']})"
        words.append(w + ("+relu" if op["relu"] and t != "relu" else ""))
    return (f"D={config['sdf_size']} L={config['latent_size']} N={config['batch_size']} tsdf={config['tsdf']}: "
            + " ".join(words))


@functools.lru_cache(maxsize=None)
def case(seed):
    """the first sub-draw of `seed` that ``parameter_shapes`` accepts and ``conditions`` hold for; None if none of
    SUB_DRAWS does (tests/test_vae_train_cases_cpu.py asserts there is one for every default seed)"""
    from sdfest_amd.train import parameter_shapes
    for sub in range(SUB_DRAWS):
        config = draw(seed, sub)
        try:
            parameter_shapes(config)
        except ValueError:
            continue
        c = setup(f"seed {seed}", config, seed, sub)
        if accepted(c.report):
            return c
    return None
