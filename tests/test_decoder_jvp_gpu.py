"""GPU: ``sdfr_decoder_jvp`` -- the decoder's forward-mode derivative w.r.t. the latent -- against ``torch.func.jvp`` of
the float64 layer walk (tests/shape_information_twin.py), on catalogue cases of tests/decoder_cases.py (their committed
sub-draws: every ReLU input is clear of 0, so the fp32 and float64 masks agree) with T = 1 and 3 seeded tangents, and on
the trained mug decoder with the identity basis (T = 8).

Bound: every tangent volume within max(1e-4, 10 x the committed torch-fp32 floor) of its largest float64
entry; the adjoint identity <G, J t> = <J^T G, t> against the existing ``sdfr_decoder_backward_latent`` on the same tape
within the same bound applied to sum |G . J t|.  The bitwise properties: zero padding, the same bits on every call and
after a workspace of 0xFF bytes, row n of the batch = its N = 1 call, enforce_tsdf zeroes exactly the clamped voxels."""
import functools

import numpy as np
import pytest
import torch

import shape_information_twin as st
from test_decoder_edges_gpu import fresh, workspace

pytestmark = pytest.mark.gpu


class Jvp:
    """the C entry points on one case's decoder, on fresh buffers"""

    def __init__(self, name, T):
        from sdfest_amd import SDFDecoder, _lib
        self.name, self.T, self.Tp = name, T, (T + 3) & ~3
        self.spec, self.state, z, tan = st.jvp_inputs(name, T)
        s = self.spec
        self.dec = SDFDecoder(s["volume"], s["latent"], s["fc"], s["conv"], tsdf=s["tsdf"], state_dict=self.state)
        for k, v in s["opts"].items():
            self.dec.set_option(k, v)
        self.L, self.h, self.check_rc = self.dec._L, self.dec._h, _lib.check
        self.N, self.vox = len(z), s["volume"] ** 3
        self.z = torch.tensor(z, device="cuda")
        self.tan = None if tan is None else torch.tensor(tan, device="cuda")

    def forward(self, clamp, z=None):
        z = self.z if z is None else z
        N = z.shape[0]
        tape = fresh(self.L.sdfr_decoder_tape_bytes(self.h, N) // 4)
        out = fresh(N * self.vox)
        ws = workspace(self.L.sdfr_decoder_workspace_bytes(self.h, N))
        self.check_rc(self.L.sdfr_decoder_forward(self.h, z.data_ptr(), N, int(clamp), out.data_ptr(), tape.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), None), "sdfr_decoder_forward")
        torch.cuda.synchronize()
        return out, tape

    def jvp(self, tape, out=None, z=None, tan=None, fill=None):
        z = self.z if z is None else z
        tan = self.tan if tan is None else tan
        N = z.shape[0]
        need = self.L.sdfr_decoder_jvp_workspace_bytes(self.h, N, self.T)
        assert need > 0
        ws = workspace(need)
        if fill is not None:
            ws.fill_(fill)
        jac = fresh(N * self.vox * self.Tp)
        jac.fill_(float("nan"))
        rc = self.L.sdfr_decoder_jvp(self.h, z.data_ptr(), tape.data_ptr(), None if out is None else out.data_ptr(),
                                     None if tan is None else tan.data_ptr(), N, self.T, int(out is not None),
                                     jac.data_ptr(), ws.data_ptr(), ws.numel(), None)
        self.check_rc(rc, "sdfr_decoder_jvp")
        torch.cuda.synchronize()
        return jac.reshape(N, self.vox, self.Tp)


@functools.lru_cache(maxsize=None)
def run(name, T):
    """(calls, tape, jac) of the unclamped call, made once per case"""
    J = Jvp(name, T)
    _, tape = J.forward(False)
    return J, tape, J.jvp(tape)


@pytest.mark.parametrize("name,T", st.jvp_case_ids())
def test_matches_float64_and_the_vjp(name, T):
    J, tape, jac = run(name, T)
    D = J.spec["volume"]
    got = jac[:, :, :T].permute(0, 2, 1).reshape(J.N, T, D, D, D).cpu().numpy()
    _, ref = st.jvp_reference(name, T)
    bound = st.jvp_bound(name, T)
    assert np.isfinite(got).all()
    err = st.row_error(got, ref)
    print(f"SHARE {name} T={T}: jac {err:.2e} of the largest float64 entry, {err / bound:.3f} of the bound {bound:.1e}")
    assert err <= bound, (name, T, err, bound)
    # <G, J t> = <J^T G, t>, J^T G from the VJP on the same tape
    rng = np.random.default_rng(3)
    G = torch.tensor(rng.normal(size=(J.N, J.vox)).astype(np.float32), device="cuda")
    g_z = fresh(J.z.numel())
    ws = workspace(J.L.sdfr_decoder_backward_workspace_bytes(J.h, J.N))
    J.check_rc(J.L.sdfr_decoder_backward_latent(J.h, J.z.data_ptr(), tape.data_ptr(), G.data_ptr(), J.N, g_z.data_ptr(),
                                                ws.data_ptr(), ws.numel(), None), "sdfr_decoder_backward_latent")
    torch.cuda.synchronize()
    tan = np.broadcast_to(np.eye(T), (J.N, T, T)) if J.tan is None else J.tan.cpu().numpy().astype(np.float64)
    Jt = jac[:, :, :T].cpu().numpy().astype(np.float64)
    G64 = G.cpu().numpy().astype(np.float64)
    lhs = np.einsum("nv,nvt->nt", G64, Jt)
    rhs = np.einsum("nl,ntl->nt", g_z.reshape(J.N, -1).cpu().numpy().astype(np.float64), tan)
    yard = np.einsum("nv,nvt->nt", np.abs(G64), np.abs(Jt))
    share = float(np.max(np.abs(lhs - rhs) / yard))
    print(f"SHARE {name} T={T}: adjoint {share:.2e} of sum |G . J t|, {share / bound:.3f} of the bound")
    assert share <= bound, (name, T, share)


@pytest.mark.parametrize("name,T", st.jvp_case_ids())
def test_bitwise_properties(name, T):
    J, tape, jac = run(name, T)
    assert T == J.Tp or not jac[:, :, T:].any().item()                      # the padding columns: exactly zero
    assert not torch.isnan(jac).any().item()                                 # ... and every entry was written
    assert torch.equal(J.jvp(tape), jac)                                     # two calls
    assert torch.equal(J.jvp(tape, fill=0xFF), jac)                          # the workspace may hold anything
    for n in sorted({0, J.N // 2, J.N - 1}):                                 # row n of the batch = its N = 1 call
        z1 = J.z[n:n + 1].contiguous()
        _, tape1 = J.forward(False, z1)
        one = J.jvp(tape1, z=z1, tan=None if J.tan is None else J.tan[n:n + 1].contiguous())
        assert torch.equal(one[0], jac[n]), (name, n)


@pytest.mark.parametrize("name", ["mix_4_to_2_k5_relu_last", "swap_6_to_5_clamp"])
def test_enforce_tsdf_zeroes_exactly_the_clamped_voxels(name):
    T = 3
    J, _, jac = run(name, T)
    out, tape = J.forward(True)
    t = 1.0 if J.spec["tsdf"] is True else float(J.spec["tsdf"])
    clamped = J.jvp(tape, out=out)
    on = (out.reshape(J.N, J.vox).abs() >= t)
    print(f"{name}: {int(on.sum())} of {on.numel()} voxels on the clamp at {t}")
    assert int(on.sum()) < on.numel()
    if name == "mix_4_to_2_k5_relu_last":      # (tsdf = 0.3 does cut into this case's volume; 1.0 leaves the other whole)
        assert int(on.sum()) > 0
    assert not clamped[on].any().item()
    assert torch.equal(clamped[~on], jac[~on])


def test_argument_errors():
    from sdfest_amd import _lib
    J, tape, _ = run("single_default", 3)
    INVALID, NULL, WORKSPACE = (_lib.ABI[k] for k in ("SDFR_E_INVALID", "SDFR_E_NULL", "SDFR_E_WORKSPACE"))
    L, h, q = J.L, J.h, tape.data_ptr()
    size = L.sdfr_decoder_jvp_workspace_bytes
    assert size(h, 1, 0) == 0 and size(h, 1, 23) == 0 and size(h, 0, 3) == 0 and size(h, 65535, 2) == 0
    need = size(h, 1, 3)
    call = lambda **kw: L.sdfr_decoder_jvp(*[kw.get(k, v) for k, v in dict(
        h=h, z=q, tape=q, out=None, tan=q, N=1, T=3, clamp=0, jac=q, ws=q, bytes=need, stream=None).items()])
    for kw, rc in ((dict(T=0), INVALID), (dict(T=23), INVALID), (dict(N=0), INVALID), (dict(N=65535, T=2), INVALID),
                   (dict(tan=None), INVALID),                       # the identity basis needs T == latent (4)
                   (dict(z=None), NULL), (dict(tape=None), NULL), (dict(jac=None), NULL), (dict(ws=None), NULL),
                   (dict(jac=q + 4), INVALID), (dict(bytes=need - 1), WORKSPACE)):
        assert call(**kw) == rc and b"sdfr_decoder_jvp" in L.sdfr_last_error(), (kw, L.sdfr_last_error())
    with pytest.raises(RuntimeError):
        J.dec.jvp(J.z, torch.zeros((1, 23, 4), device="cuda"))


def test_python_surface_matches_the_c_call():
    from sdfest_amd import SDFDecoder
    J, _, jac = run(st.MUG, 8)
    sdf, got = J.dec.jvp(J.z)
    assert sdf.shape == (1, 1, 64, 64, 64) and got.shape == (1, 64 ** 3, 8) and torch.equal(got, jac)
    with torch.no_grad():
        assert torch.equal(sdf, J.dec.decode(J.z)) or (sdf - J.dec.decode(J.z)).abs().max().item() <= 1e-6
    vols = SDFDecoder.tangent_volumes(got, 8)
    assert vols.shape == (1, 8, 64, 64, 64) and vols.data_ptr() == got.data_ptr()
    assert torch.equal(vols[0, 3].reshape(-1), got[0, :, 3])
    # explicit tangents: the identity basis spelled out, and a T = 1 direction as a combination of its columns
    eye = torch.eye(8, device="cuda")[None].contiguous()
    assert torch.equal(J.dec.jvp(J.z, eye)[1], got)
