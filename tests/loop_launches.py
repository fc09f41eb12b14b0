"""The launch sequence of every form of the render-and-compare loops, as a log of the C ABI calls of one run: the case
list and the recorder that tests/test_loop_launches_gpu.py and tools/record_loop_launches.py share.  The committed log
(tests/golden/loop_launch_sequences.json) pins what a loop object issues -- which entry points, in which order, with
which small arguments -- so that host-side changes to sdfest_amd/pipeline.py cannot move a launch unnoticed.

A case builds its loop on the smallest loop scene of the repository (tests/loop_decoders.py: 64x48 images, 2 views, the
first decoder with a narrow Linear stack) and runs ``max_iterations = 2`` eagerly (``use_graph=False``) under a
stand-in for ``sdfest_amd._lib.lib`` that forwards every call.  Only the run is logged -- the priming and two whole
iterations -- not the construction.  Per call: the entry point's name and, per argument, None, a float verbatim, an
int below 2^20 verbatim (V, W, H, flags, stages, small offsets, device and default stream), or "ptr" for anything else.
"""
import contextlib
import functools
import itertools
import json
import os

import numpy as np
import torch

import loop_decoders as D

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE_PATH = os.path.join(HERE, "golden", "loop_launch_sequences.json")
NAME = next(n for n in D.NAMES if D.FAMILY[n]["narrow"])      # the first decoder whose Linear stack is narrow
ITERATIONS = 2
CONSTRAINT = ([0.0, 0.0, 1.0], [0.0, 1.0, 0.0], 0.5)          # source, target, weight (simple_setup.py:164-175)
SMALL_VERBATIM = 1 << 20


def _spell(a):
    if a is None:
        return None
    if isinstance(a, float):
        return a
    if isinstance(a, int) and 0 <= a < SMALL_VERBATIM:       # (bool included: it is an int)
        return int(a)
    return "ptr"


class Recorder:
    """stands in for the loaded library: forwards every call, logs those made while ``on``"""

    def __init__(self, lib):
        self._lib, self.on, self.log = lib, False, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("sdfr_"):
            return fn

        def call(*args):
            if self.on:
                self.log.append([name] + [_spell(a) for a in args])
            return fn(*args)
        return call


@contextlib.contextmanager
def recording():
    """``sdfest_amd._lib.lib`` hands out a Recorder for the duration of the block"""
    from sdfest_amd import _lib
    real = _lib.lib
    rec = Recorder(real())
    _lib.lib = lambda: rec
    try:
        yield rec
    finally:
        _lib.lib = real


# ---- the cases -------------------------------------------------------------------------------------------------------

def _modes():
    from sdfest_amd.differentiable_renderer import BWD_SMALL_TILES, SDF_GRAD_DETERMINISTIC
    return {"mode0": 0, "det_small": SDF_GRAD_DETERMINISTIC | BWD_SMALL_TILES}


# form -> constructor arguments (tests/test_loop_decoders_gpu.py::FORMS) and whether it runs without shape optimisation
FORMS = {
    "separate_fused_loss": (dict(merge_launches=False, fuse_depth_loss=True), True),
    "separate_loss_kernels": (dict(merge_launches=False, fuse_depth_loss=False), True),
    "tail": (dict(form="tail", fused_render=False), True),
    "one_launch": (dict(fused_render=True, fc_in_tail=False), True),
    "fc_in_tail": (dict(fused_render=True, fc_in_tail=True), False),
}


def cases():
    """{case id: (kind, keyword arguments)}; kind: "fused" | "oversize" | "multi" """
    out = {}
    for (form, (kw, pose_only)), shape, con, inl in itertools.product(FORMS.items(), (True, False), (False, True),
                                                                      (False, True)):
        if shape or pose_only:
            out[f"{form}-shape{int(shape)}-con{int(con)}-inl{int(inl)}"] = (
                "fused", dict(kw, shape_optimization=shape, constraint=con, track_inliers=inl))
    for exchange, mode, shape, con, inl in itertools.product(("sdf", "latent"), _modes().items(), (True, False),
                                                             (False, True), (False, True)):
        out[f"records-{exchange}-{mode[0]}-shape{int(shape)}-con{int(con)}-inl{int(inl)}"] = (
            "fused", dict(form="records", exchange=exchange, sdf_grad_mode=mode[1], shape_optimization=shape,
                          constraint=con, track_inliers=inl))
    # a parameter vector of 257 (loop_decoders.OVERSIZE): the separate launches with both backward passes in ONE
    # launch, the variant no decoder of 256 parameters or fewer reaches
    for shape in (True, False):
        out[f"separate_merged-shape{int(shape)}-con1-inl1"] = (
            "oversize", dict(shape_optimization=shape, constraint=True, track_inliers=True))
    for V, shape, inl in itertools.product((1, 2), (True, False), (False, True)):
        out[f"multi-K2-V{V}-shape{int(shape)}-inl{int(inl)}"] = (
            "multi", dict(views=V, shape_optimization=shape, track_inliers=inl))
    return out


T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device="cuda")


def _camera():
    from sdfest_amd import Camera
    return Camera(D.W, D.H, D.F, D.F, D.W / 2, D.H / 2, pixel_center=0.5)


def _config():
    return {"threshold": D.THRESHOLD, "max_iterations": ITERATIONS, "depth_weight": D.DEPTH_WEIGHT,
            "pc_weight": D.PC_WEIGHT}


def _run_fused(dec, sc, z0, kw):
    from sdfest_amd.pipeline import FusedRenderAndCompare
    kw = dict(kw)
    con = tuple(T(x) if isinstance(x, list) else x for x in CONSTRAINT) if kw.pop("constraint") else None
    loop = FusedRenderAndCompare(dec, _camera(), _config(), T(sc["obs"]), T(sc["cam_pos"]), T(sc["cam_quat"]),
                                 point_constraint=con, **kw)
    return loop, (T(sc["p0"][None]), T(sc["q0"][None]), T([sc["s0"]]), z0)


def _run_multi(dec, kw):
    from sdfest_amd.pipeline import MultiObjectRenderAndCompare
    V = kw["views"]
    scs = [D.scene(NAME, f"object{k}") for k in range(2)]
    views = D.scene(NAME, "views")
    loop = MultiObjectRenderAndCompare(dec, _camera(), _config(), 2, **kw)
    if V == 1:
        loop.rebind(T(np.concatenate([s["obs"] for s in scs])))
    else:      # both objects against the two-view observation, from its two cameras
        loop.rebind(T(np.stack([views["obs"]] * 2)), T(views["cam_pos"]), T(views["cam_quat"]))
    return loop, (T(np.stack([s["p0"] for s in scs])), T(np.stack([s["q0"] for s in scs])),
                  T([s["s0"] for s in scs]), T(np.stack([s["z0"] for s in scs])))


def record_case(kind, kw, decoders):
    """the log of one case's run; `decoders`: a dict the caller keeps, so that a decoder is built once"""
    if kind == "oversize":
        from sdfest_amd import SDFDecoder
        spec = D.OVERSIZE
        if "oversize" not in decoders:
            decoders["oversize"] = SDFDecoder.from_config(D.config(spec), D.state_dict(spec), sdf_size=spec["volume"])
        dec, sc = decoders["oversize"], D.scene("latent248")       # (any observation will do)
        z0 = T(0.3 * np.random.default_rng(3).normal(size=(1, spec["latent"])))
    else:
        if NAME not in decoders:
            decoders[NAME] = D.gpu_decoder(NAME)
        dec, sc = decoders[NAME], D.scene(NAME)
        z0 = T(sc["z0"][None])
    with recording() as rec:
        loop, args = _run_multi(dec, kw) if kind == "multi" else _run_fused(dec, sc, z0, kw)
        rec.on = True
        loop(*args, use_graph=False)
        rec.on = False
    torch.cuda.synchronize()
    return rec.log


@functools.lru_cache(maxsize=None)
def load_fixture():
    with open(FIXTURE_PATH) as f:
        return json.load(f)
