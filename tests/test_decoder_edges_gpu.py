"""GPU: every launch form the decoder's planner (sdfest_amd/csrc/decoder_plan.hpp) can choose and every entry point of the
decoder's VJP, on the cases of tests/decoder_cases.py, against float64 (test_decoder_gpu.torch_decoder, the layer sequence
of sdf_vae.py:171-259): the forward without a tape, with one and with the tsdf clamp; sdfr_decoder_forward_stage; the
latent VJP; its _deferred, _deferred_batch and _deferred_scaled forms; out, tape and grad_out 4 bytes past 16-byte
alignment.  Each case asserts that its plan holds the forms it exists for, and the catalogue together reaches every
SDFR_DECODER_STEP_* code of include/sdfr.h.

Bound: max(1e-4, 10 x the committed fp32 floor of the tensor) in units of its largest float64 entry (the rule of
test_loop_decoders_gpu.py); the cases are drawn so that no ReLU decision is in doubt (decoder_cases.conditions)."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decoder_cases as dc
import test_decoder_gpu as D

pytestmark = pytest.mark.gpu

EDGES = list(dc.CATALOGUE)
SEEDS = [f"seed {s}" for s in dc.default_seeds()]
N1_EDGES = [n for n in EDGES if dc.CATALOGUE[n]["N"] == 1]


# ---- the float64 statement, once per case ------------------------------------------------------------------------------
def _leading(state, fc, z):
    """the Linear layers in front of the wide one, as torch_decoder writes them"""
    P = lambda key: torch.tensor(state[key]).to(torch.float64)
    for i in range(len(fc) - 1):
        z = F.relu(F.linear(z, P(f"decoder._fc_layers.{i}.weight"), P(f"decoder._fc_layers.{i}.bias")))
    return z


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64: out (and its yardstick), the clamped out, g_z, t_mid = d/d(the wide layer's input), and t_mid of the
    scaled form's sums; torch_decoder whole for out and g_z, and from the wide layer on for t_mid"""
    c = dc.case(name)
    s = c.spec
    fc, conv, volume, n_fc = s["fc"], s["conv"], s["volume"], len(s["fc"])
    G = torch.tensor(c.G, dtype=torch.float64)
    z = torch.tensor(c.z, dtype=torch.float64, requires_grad=True)
    out = D.torch_decoder(c.state, fc, conv, volume, z)
    (g_z,) = torch.autograd.grad(out, [z], G)
    r = {"out": out.detach().numpy(), "g_z": g_z.numpy()}
    pre = out if not conv[-1]["relu"] else D.torch_decoder(c.state, fc, conv[:-1] + [dict(conv[-1], relu=False)], volume, z)
    r["scale"] = float(pre.detach().abs().max())       # a ReLU'd last layer: the size of what that ReLU saw
    t = dc.clamp_of(s)
    if t is not None:
        r["clamp"] = np.clip(r["out"], -t, t)
        r["clamp_scale"] = float(np.abs(np.clip(pre.detach().numpy(), -t, t)).max())
    # from the wide layer on: torch_decoder with the wide layer as its only Linear layer, fed its input
    h = _leading(c.state, fc, z.detach()).detach().requires_grad_(True)
    tail_state = {k: v for k, v in c.state.items() if not k.startswith("decoder._fc_layers.")}
    tail_state["decoder._fc_layers.0.weight"] = c.state[f"decoder._fc_layers.{n_fc - 1}.weight"]
    tail_state["decoder._fc_layers.0.bias"] = c.state[f"decoder._fc_layers.{n_fc - 1}.bias"]
    tail = D.torch_decoder(tail_state, fc[-1:], conv, volume, h)
    r["t_mid"] = torch.autograd.grad(tail, [h], G, retain_graph=True)[0].numpy()
    r["scaled"] = {}
    for n, sc in c.scaled.items():
        g = torch.tensor(dc.scaled_sum(sc)).reshape(G.shape)
        (tm,) = torch.autograd.grad(tail, [h], g, retain_graph=True)
        r["scaled"][n] = tm.numpy()
    return r


def finish(name, t_mid):
    """the leading Linear layers' VJP in float64 from a t_mid: what sdfr_loop_tail[_objects] finishes on the GPU"""
    c = dc.case(name)
    z = torch.tensor(c.z, dtype=torch.float64, requires_grad=True)
    h = _leading(c.state, c.spec["fc"], z)
    if not h.requires_grad:         # one Linear layer: its input is z itself
        return np.asarray(t_mid, np.float64)
    (g,) = torch.autograd.grad(h, [z], torch.tensor(np.asarray(t_mid, np.float64)))
    return g.numpy()


def check(what, got, ref, scale, bound):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    got = got.reshape(ref.shape)
    assert np.isfinite(got).all(), what
    err = float(np.abs(got.astype(np.float64) - ref).max()) / max(scale, 1e-30)
    print(f"SHARE {what}: {err:.2e} of the largest float64 entry, {err / bound:.3f} of the bound {bound:.1e}")
    assert err <= bound, f"{what}: {err:.2e} > {bound:.1e}"


# ---- the C entry points, on fresh buffers --------------------------------------------------------------------------
def fresh(n, offset=0):
    """n floats on the GPU, `offset` floats past the start of a fresh allocation (256-byte aligned)"""
    return torch.empty(n + offset, dtype=torch.float32, device="cuda")[offset:]


def workspace(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


class Calls:
    def __init__(self, name):
        from sdfest_amd import SDFDecoder, _lib
        self.name, self.c = name, dc.case(name)
        s = self.c.spec
        self.dec = SDFDecoder(s["volume"], s["latent"], s["fc"], s["conv"], tsdf=s["tsdf"], state_dict=self.c.state)
        self.L, self.h, self.check_rc = self.dec._L, self.dec._h, _lib.check
        self.N, self.vox = s["N"], s["volume"] ** 3
        self.win = s["fc"][-2]["out"] if len(s["fc"]) > 1 else s["latent"]
        self.z = torch.tensor(self.c.z, device="cuda")
        self.G = torch.tensor(self.c.G, device="cuda")

    @contextlib.contextmanager
    def options(self):
        """the case's option settings on the handle for the duration"""
        old = {}
        try:
            for k, v in self.c.spec["opts"].items():
                old[k] = self.dec.set_option(k, v)
            yield
        finally:
            for k, v in old.items():
                self.dec.set_option(k, v)

    def tape(self, offset=0):
        return fresh(self.L.sdfr_decoder_tape_bytes(self.h, self.N) // 4, offset)

    def forward(self, clamp=False, tape=None, offset=0):
        out = fresh(self.N * self.vox, offset)
        ws = workspace(self.L.sdfr_decoder_workspace_bytes(self.h, self.N))
        rc = self.L.sdfr_decoder_forward(self.h, self.z.data_ptr(), self.N, int(clamp), out.data_ptr(),
                                         None if tape is None else tape.data_ptr(), ws.data_ptr(), ws.numel(), None)
        self.check_rc(rc, "sdfr_decoder_forward")
        torch.cuda.synchronize()
        return out

    def stages(self, clamp, tape):
        """stage 1 (the Linear stack into the tape), then stage 2 (the convolutional part from there)"""
        out = fresh(self.N * self.vox)
        ws = workspace(self.L.sdfr_decoder_workspace_bytes(self.h, self.N))
        rc = self.L.sdfr_decoder_forward_stage(self.h, self.z.data_ptr(), self.N, int(clamp), None, tape.data_ptr(),
                                               ws.data_ptr(), ws.numel(), None, 1)
        self.check_rc(rc, "sdfr_decoder_forward_stage(1)")
        rc = self.L.sdfr_decoder_forward_stage(self.h, None, self.N, int(clamp), out.data_ptr(), tape.data_ptr(),
                                               ws.data_ptr(), ws.numel(), None, 2)
        self.check_rc(rc, "sdfr_decoder_forward_stage(2)")
        torch.cuda.synchronize()
        return out

    def grad_out(self, offset=0):
        g = fresh(self.G.numel(), offset)
        g.copy_(self.G.reshape(-1))
        return g

    def backward(self, tape, grad_out):
        g_z = fresh(self.z.numel())
        ws = workspace(self.L.sdfr_decoder_backward_workspace_bytes(self.h, self.N))
        rc = self.L.sdfr_decoder_backward_latent(self.h, self.z.data_ptr(), tape.data_ptr(), grad_out.data_ptr(), self.N,
                                                 g_z.data_ptr(), ws.data_ptr(), ws.numel(), None)
        self.check_rc(rc, "sdfr_decoder_backward_latent")
        torch.cuda.synchronize()
        return g_z.reshape(self.z.shape)

    def _t_mid(self, ws, ptr, rows):
        """[rows][width of the wide layer's input] at *t_mid, inside the workspace (as sdfr_loop_tail reads it)"""
        off = ptr.value - ws.data_ptr()
        n = rows * self.win * 4
        assert off % 4 == 0 and 0 <= off and off + n <= ws.numel(), (off, n, ws.numel())
        return ws[off:off + n].view(torch.float32).reshape(rows, self.win).clone()

    def deferred(self, tape, grad_out, batch):
        ws = workspace(self.L.sdfr_decoder_backward_workspace_bytes(self.h, self.N))
        ptr = ctypes.c_void_p()
        if batch:
            rc = self.L.sdfr_decoder_backward_latent_deferred_batch(self.h, self.z.data_ptr(), tape.data_ptr(),
                                                                    grad_out.data_ptr(), self.N, ws.data_ptr(), ws.numel(),
                                                                    None, ctypes.byref(ptr))
        else:
            rc = self.L.sdfr_decoder_backward_latent_deferred(self.h, self.z.data_ptr(), tape.data_ptr(),
                                                              grad_out.data_ptr(), ws.data_ptr(), ws.numel(), None,
                                                              ctypes.byref(ptr))
        self.check_rc(rc, "sdfr_decoder_backward_latent_deferred" + ("_batch" if batch else ""))
        torch.cuda.synchronize()
        return self._t_mid(ws, ptr, self.N)

    def deferred_scaled(self, tape, grad_out, parts, count, weight):
        ws = workspace(self.L.sdfr_decoder_backward_workspace_bytes(self.h, 1))
        ptr = ctypes.c_void_p()
        rc = self.L.sdfr_decoder_backward_latent_deferred_scaled(
            self.h, self.z.data_ptr(), tape.data_ptr(), grad_out.data_ptr(), parts.data_ptr(), parts.shape[0],
            count.data_ptr(), float(weight), ws.data_ptr(), ws.numel(), None, ctypes.byref(ptr))
        self.check_rc(rc, "sdfr_decoder_backward_latent_deferred_scaled")
        torch.cuda.synchronize()
        return self._t_mid(ws, ptr, 1)

    def plans(self):
        """every plan the tests below launch: pass -> step names (the case's options must be set)"""
        N, d, s = self.N, self.dec, self.c.spec
        p = {"forward": d.launch_plan(N), "taped forward": d.launch_plan(N, tape=True),
             "stage 1": d.launch_plan(N, stages=1), "stage 2": d.launch_plan(N, stages=2),
             "vjp": d.launch_plan(N, vjp=True), "deferred": d.launch_plan(N, vjp=True, deferred=True)}
        if s["tsdf"] is not False:
            p["clamped forward"] = d.launch_plan(N, enforce_tsdf=True)
            p["clamped taped forward"] = d.launch_plan(N, tape=True, enforce_tsdf=True)
            p["clamped stage 2"] = d.launch_plan(N, stages=2, enforce_tsdf=True)
        if N == 1:
            p["scaled, one view"] = d.launch_plan(1, vjp=True, scaled_views=1)
            p["scaled, several views"] = d.launch_plan(1, vjp=True, scaled_views=2)
        return p


# ---- the passes -------------------------------------------------------------------------------------------------------
def run_forward(name):
    k, ref = Calls(name), reference(name)
    with k.options():
        plain = k.forward()
        taped = k.forward(tape=k.tape())
        assert torch.equal(plain, taped), f"{name}: the taped forward is not the inference forward bit for bit"
        check(f"{name} forward", plain, ref["out"], ref["scale"], dc.bound(k.c, "out"))
        for clamp in ((False, True) if "clamp" in ref else (False,)):
            tape = k.tape()
            whole = k.forward(clamp=clamp, tape=tape)
            staged = k.stages(clamp, k.tape())
            assert torch.equal(staged, whole), f"{name}: stage 1 + stage 2 (clamp {clamp}) is not sdfr_decoder_forward"
        if "clamp" in ref:
            clamped = k.forward(clamp=True)
            check(f"{name} clamped forward", clamped, ref["clamp"], ref["clamp_scale"], dc.bound(k.c, "clamp"))
        # out and tape 4 bytes past 16-byte alignment
        check(f"{name} forward, misaligned out + tape", k.forward(tape=k.tape(1), offset=1), ref["out"], ref["scale"],
              dc.bound(k.c, "out"))


def run_vjp(name, deferred_single):
    k, ref = Calls(name), reference(name)
    gz_ref, tm_ref = ref["g_z"], ref["t_mid"]
    with k.options():
        tape = k.tape()
        k.forward(tape=tape)
        g = k.grad_out()
        check(f"{name} backward_latent", k.backward(tape, g), gz_ref, np.abs(gz_ref).max(), dc.bound(k.c, "g_z"))
        for batch in ((True, False) if deferred_single and k.N == 1 else (True,)):
            form = "_deferred_batch" if batch else "_deferred"
            tm = k.deferred(tape, g, batch)
            check(f"{name} {form} t_mid", tm, tm_ref, np.abs(tm_ref).max(), dc.bound(k.c, "t_mid"))
            check(f"{name} {form} t_mid finished in float64", finish(name, tm.cpu().numpy()), gz_ref, np.abs(gz_ref).max(),
                  dc.bound(k.c, "g_z"))
        # tape and grad_out 4 bytes past 16-byte alignment (the forward's out too)
        tape_m = k.tape(1)
        k.forward(tape=tape_m, offset=1)
        check(f"{name} backward_latent, misaligned tape + grad_out", k.backward(tape_m, k.grad_out(1)), gz_ref,
              np.abs(gz_ref).max(), dc.bound(k.c, "g_z"))


@pytest.mark.parametrize("name", EDGES)
def test_plan_holds_the_case_forms(name):
    k = Calls(name)
    with k.options():
        plans = k.plans()
    for what, plan in plans.items():
        print(f"{name} {what}: {' '.join(plan)}")
    took = set().union(*plans.values())
    missing = k.c.spec["forms"] - took
    assert not missing, f"{name} ({dc.describe(k.c.spec)}) no longer takes {sorted(missing)}"


def test_catalogue_reaches_every_step_code():
    """the union of the catalogue's plans holds every SDFR_DECODER_STEP_* code of include/sdfr.h but those listed as
    unreachable; and both ways the scaled form sums its volumes: in its first stage, and in a launch of its own"""
    from sdfest_amd import SDFDecoder
    by = {code: [] for code in SDFDecoder.STEPS}
    sums = set()
    for name in EDGES:
        k = Calls(name)
        with k.options():
            plans = k.plans()
        for plan in plans.values():
            for code, step in SDFDecoder.STEPS.items():
                if step in plan and name not in by[code]:
                    by[code].append(name)
        if "scaled, one view" in plans:
            sums.add("scaled_combine" in plans["scaled, one view"])
            assert "scaled_combine" in plans["scaled, several views"], name
    for code, names in sorted(by.items()):
        print(f"{code:2d} {SDFDecoder.STEPS[code]}: {', '.join(names) or dc.UNREACHABLE.get(code, '-')}")
    assert sorted(SDFDecoder.STEPS) == list(range(1, 32))
    assert not [c for c, n in by.items() if not n and c not in dc.UNREACHABLE], "step codes no case reaches"
    assert not [c for c in dc.UNREACHABLE if by[c]], "a step listed as unreachable is reached"
    assert sums == {True, False}, "the scaled form's sum on load and as its own launch"


@pytest.mark.parametrize("name", EDGES)
def test_forward_forms_against_float64(name):
    run_forward(name)


@pytest.mark.parametrize("name", EDGES)
def test_vjp_entries_against_float64(name):
    run_vjp(name, deferred_single=True)


@pytest.mark.parametrize("name", N1_EDGES)
def test_deferred_scaled_against_float64(name):
    """grad_out + sum_v k_v grad_scaled[v] for 1, 2, 7 and 64 views, one of them with count 0 over values of 1e30; every
    volume is zero once the call has read it"""
    k, ref = Calls(name), reference(name)
    with k.options():
        tape = k.tape()
        k.forward(tape=tape)
        for n, sc in k.c.scaled.items():
            g = torch.tensor(sc["grad_out"], device="cuda").reshape(-1).contiguous()
            parts = torch.tensor(sc["parts"], device="cuda").contiguous()
            count = torch.tensor(sc["count"], device="cuda")
            assert g.data_ptr() % 16 == 0 and parts.data_ptr() % 16 == 0
            tm = k.deferred_scaled(tape, g, parts, count, sc["weight"])
            check(f"{name} _deferred_scaled ({n} views) t_mid", tm, ref["scaled"][n], np.abs(ref["scaled"][n]).max(),
                  dc.bound(k.c, "scaled"))
            assert not g.any() and not parts.any(), f"{name}, {n} views: a volume is not zero-filled"


@pytest.mark.parametrize("name", SEEDS)
def test_random_architecture_against_float64(name):
    print(name, dc.describe(dc.case(name).spec))
    run_forward(name)
    run_vjp(name, deferred_single=False)
