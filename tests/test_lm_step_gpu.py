"""GPU: ``sdfr_lm_step`` against its numpy float64 twin (tests/lm_twin.py) on synthetic Gram matrices -- no render.

K = 3 objects, V in {1, 2, 64} views, T in {0, 1, 8, 22} latent directions.  The Gram matrices are F^T F of random
float64 features (so each is positive semi-definite with an exact count), evaluated nowhere: the step never asks where
they come from.  What the kernel decides (accept / reject, status, lambda, the costs) equals the twin's exactly; what it
solves matches to the bounds below."""
import numpy as np
import pytest
import torch

import lm_twin as tw
from test_lm_cpu import degenerate_zero_latent_column

pytestmark = pytest.mark.gpu

K = 3
CASES = [(V, T) for V in (1, 2, 64) for T in (0, 1, 8, 22)]
# ||A delta + g|| <= SOLVE (||A|| ||delta|| + ||g||): n eps for n = 29 in float64 is 3e-15, a margin of some 300 for
# the growth of the Cholesky factorisation and the different summation order of the views
SOLVE = 1e-12
EXACT = [tw.LAMBDA, tw.COST, tw.COUNT, tw.STATUS, tw.ACCEPTED, tw.REJECTED, tw.ACTUAL, tw.COST_INIT, tw.COUNT_INIT,
         tw.LAST_ACCEPT, tw.COST_TRIAL, tw.COUNT_TRIAL]


def random_grams(rng, V, T, pixels=40, scale=1.0, k=K):
    """(k, V, F, F): F^T F of `pixels` rows f = (d0 .. d7, s.., r, 1) per view; `scale` multiplies the residual column"""
    F = 10 + T
    f = rng.standard_normal((k, V, pixels, F))
    f[..., 8 + T] *= scale
    f[..., 9 + T] = 1.0
    return np.einsum("kvpi,kvpj->kvij", f, f)


def random_rows(rng, T, extra=0, k=K):
    rows = np.zeros((k, 8 + T + extra))
    rows[:, 0:3] = rng.uniform(-0.3, 0.3, (k, 3)) + [0.0, 0.0, -1.0]
    rows[:, 3:7] = rng.standard_normal((k, 4)) * 1.3          # (not normalised: the loop's rows are not either)
    rows[:, 7] = rng.uniform(0.1, 0.3, k)
    rows[:, 8:] = 0.5 * rng.standard_normal((k, T + extra))
    return rows.astype(np.float32)


def cameras(rng, V):
    q = rng.standard_normal((V, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


class Device:
    """the kernel's buffers for k objects, poisoned with 0xFF bytes, and one call = ``sdfest_amd.lm.lm_step``"""

    def __init__(self, rows, V, T, cam_quat, **constants):
        k, n_params = rows.shape
        F = 10 + T
        poison = lambda shape, dtype: torch.full(shape, 0xFF, dtype=torch.uint8, device="cuda").view(dtype)
        self.V, self.T, self.constants = V, T, constants
        self.pt = torch.tensor(rows, device="cuda")
        self.pc = poison((k, n_params * 4), torch.float32)
        self.gc = poison((k * V, F, F * 8), torch.float64)
        self.S = poison((k, tw.STATE_DOUBLES * 8), torch.float64)
        self.step = poison((k, (7 + T) * 8), torch.float64)
        self.cq = torch.tensor(cam_quat, device="cuda")

    def __call__(self, gram, init):
        from sdfest_amd.lm import lm_step
        k = self.pt.shape[0]
        gt = torch.tensor(np.ascontiguousarray(gram).reshape(k * self.V, 10 + self.T, 10 + self.T), device="cuda")
        lm_step(gt, self.pt, self.pc, self.gc, self.S, self.cq, self.V, init, step=self.step, **self.constants)
        return self.arrays()

    def arrays(self):
        k, F = self.pt.shape[0], 10 + self.T
        return dict(trial=self.pt.cpu().numpy(), cur=self.pc.cpu().numpy(),
                    gram=self.gc.cpu().numpy().reshape(k, self.V, F, F), state=self.S.cpu().numpy(),
                    step=self.step.cpu().numpy())


def ulp32(a, b):
    """distance in float32 units in the last place of the larger magnitude (0 where the bits agree)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def check_against_twin(got, want, system, T, what):
    """bookkeeping exactly, the solve to SOLVE, the rows to 1 ulp of float32 -- plus, per row, what the solve's forward
    error can move a component by: Cholesky is backward stable, so two correct solves of A delta = -g differ by up to
    ~cond(A) eps |delta| (taken as 4 cond(A) 2^-52 max |delta|, in units of the component's float32 spacing).  For the
    well-conditioned random systems of this file that term is below 1e-3 ulp; it matters for near-singular real ones
    (tests/test_refine_gpu.py).  The scaled norm and the predicted reduction carry the same forward error."""
    S, St = got["state"], want[3]
    assert np.array_equal(S[:, EXACT], St[:, EXACT], equal_nan=True), (what, S[:, EXACT], St[:, EXACT])
    assert not S[:, 14:].any()
    assert np.array_equal(got["cur"].view(np.uint32), want[1].view(np.uint32)), what
    assert np.array_equal(got["gram"], want[2], equal_nan=True), what
    worst, slack = 0.0, np.zeros(len(system))
    for k, sys_k in enumerate(system):
        if sys_k is None:
            assert not got["step"][k].any(), what
            continue
        A, g = sys_k
        d = got["step"][k]
        res = np.linalg.norm(A @ d + g) / (np.linalg.norm(A, 2) * np.linalg.norm(d) + np.linalg.norm(g))
        worst = max(worst, res)
        assert res <= SOLVE, (what, k, res)
        forward = 4.0 * np.linalg.cond(A) * 2.0 ** -52
        assert abs(S[k, tw.STEP_NORM] - St[k, tw.STEP_NORM]) <= (1e-9 + forward) * St[k, tw.STEP_NORM], what
        assert abs(S[k, tw.PREDICTED] - St[k, tw.PREDICTED]) <= (1e-9 + forward) * (
            2.0 * abs(g @ d) + abs(d @ A @ d)) + 1e-300, what
        slack[k] = forward * np.abs(d).max()
    a32, b32 = np.asarray(got["trial"], np.float32), np.asarray(want[0], np.float32)
    u = ulp32(a32, b32)
    allowed = 1.0 + slack[:, None] / np.spacing(np.maximum(np.abs(a32), np.abs(b32)).astype(np.float32)).astype(np.float64)
    assert (u <= allowed).all(), (what, u.max(), allowed.max())
    return worst, u.max()


@pytest.mark.parametrize("V, T", CASES)
def test_steps_match_the_twin(V, T):
    """init and three further steps fed random Gram matrices whose residual shrinks and grows (accepts AND rejects):
    the decisions, lambda and the costs are the twin's exactly, the step solves the twin's system to SOLVE, the rows agree
    to 1 ulp of float32; nothing of the 0xFF poison survives; a second device run gives the same bits (reproducible),
    and object 1 run alone gives row 1's bits (row independence)."""
    rng = np.random.default_rng(1000 * V + T)
    rows, cq = random_rows(rng, T, extra=2), cameras(rng, V)
    grams = [random_grams(rng, V, T, scale=s) for s in (1.0, 0.7, 1.5, 0.5)]
    mu = 0.01 if T else 0.0
    dev, again, alone = (Device(r, V, T, cq, latent_weight=mu) for r in (rows, rows, rows[1:2]))
    pt, pc = rows.copy(), np.zeros_like(rows)
    gc, S = np.zeros_like(grams[0]), np.zeros((K, tw.STATE_DOUBLES))
    accepts, worst = [], (0.0, 0.0)
    for it, G in enumerate(grams):
        want = tw.lm_step(G, pt, pc, gc, S, cq, T, it == 0, latent_weight=mu)
        got = dev(G, it == 0)
        worst = np.maximum(worst, check_against_twin(got, want, want[5], T, (V, T, it)))
        for name, a in got.items():
            assert np.isfinite(a).all() or name == "state", (name, it)      # no poison (NaN bytes) left anywhere
        assert np.isfinite(got["state"][:, [tw.LAMBDA, tw.COST, tw.COUNT, tw.STATUS, tw.STEP_NORM, tw.PREDICTED]]).all()
        second, single = again(G, it == 0), alone(G[1:2], it == 0)
        for name in got:
            assert got[name].tobytes() == second[name].tobytes(), (name, it)
            assert got[name][1:2].tobytes() == single[name].tobytes(), (name, it)
        accepts.append(got["state"][:, tw.LAST_ACCEPT].copy())
        # the twin goes on from the DEVICE's rows: one ulp of a trial row must not compound into the next comparison
        pt, pc, gc, S = got["trial"], got["cur"], got["gram"], got["state"]
    accepts = np.array(accepts)
    print(f"V={V} T={T}: solve residual {worst[0]:.2e} (bound {SOLVE:.0e}), rows within {worst[1]:.2f} ulp, "
          f"accepts per step {accepts.sum(1).tolist()}")
    assert accepts[0].all() and accepts[1:].any() and not accepts[1:].all()      # both branches were taken


def forced_states(rng, V, T):
    """three rows that freeze: converged (a huge step_tol), stalled (lambda_max below lambda0 lambda_up, after a
    rejection) and no usable system (all-zero Gram matrices), as (constants, grams of the init call, grams after)"""
    good, worse = random_grams(rng, V, T, k=1), random_grams(rng, V, T, scale=3.0, k=1)
    return {tw.CONVERGED: (dict(step_tol=1e30), good, random_grams(rng, V, T, scale=0.3, k=1)),
            tw.STALLED: (dict(lambda0=1.0, lambda_up=10.0, lambda_max=5.0), good, worse),
            tw.NO_SYSTEM: (dict(), np.zeros_like(good), good)}


@pytest.mark.parametrize("status", [tw.CONVERGED, tw.STALLED, tw.NO_SYSTEM])
def test_frozen_rows_stay_bit_for_bit(status):
    V, T = 2, 8
    rng = np.random.default_rng(50 + status)
    constants, first, then = forced_states(rng, V, T)[status]
    rows, cq = random_rows(rng, T, k=1), cameras(rng, V)
    dev = Device(rows, V, T, cq, **constants)
    got = dev(first, True)
    want = tw.lm_step(first, rows, np.zeros_like(rows), np.zeros_like(first), np.zeros((1, 16)), cq, T, True, **constants)
    if status != tw.NO_SYSTEM:       # one more call takes it there
        assert got["state"][0, tw.STATUS] == tw.RUNNING
        want = tw.lm_step(then, got["trial"], got["cur"], got["gram"], got["state"], cq, T, False, **constants)
        got = dev(then, False)
    assert got["state"][0, tw.STATUS] == want[3][0, tw.STATUS] == status
    assert got["trial"].tobytes() == got["cur"].tobytes()
    for _ in range(3):               # whatever comes in, better or worse
        dev.pt.add_(0.25)            # (a caller scribbling on the trial row)
        after = dev(random_grams(rng, V, T, scale=rng.uniform(0.1, 3.0), k=1), False)
        for name in ("cur", "gram", "state"):
            assert after[name].tobytes() == got[name].tobytes(), name
        assert after["trial"].tobytes() == got["cur"].tobytes() and not after["step"].any()


def test_zero_latent_column_gives_a_zero_step_there():
    problem, rows = degenerate_zero_latent_column(np.random.default_rng(7))
    rows = np.array(rows, np.float32)
    got = Device(rows, problem.V, problem.T, problem.cam_quat.astype(np.float32))(problem.gram(rows), True)
    assert got["state"][0, tw.STATUS] == tw.RUNNING and np.isfinite(got["step"]).all()
    assert got["step"][0, 7 + 3] == 0.0 and np.abs(got["step"][0]).max() > 0.0
    assert got["trial"][0, 8 + 3] == got["cur"][0, 8 + 3] and np.isfinite(got["trial"]).all()


def test_all_zero_gram_is_no_system():
    rng = np.random.default_rng(8)
    rows, cq = random_rows(rng, 8), cameras(rng, 2)
    got = Device(rows, 2, 8, cq)(np.zeros((K, 2, 18, 18)), True)
    assert (got["state"][:, tw.STATUS] == tw.NO_SYSTEM).all()
    assert got["trial"].tobytes() == got["cur"].tobytes() == rows.tobytes()


def test_nan_in_a_trial_gram_is_rejected_or_no_system_on_init():
    rng = np.random.default_rng(9)
    V, T = 2, 1
    rows, cq = random_rows(rng, T), cameras(rng, V)
    good, bad = random_grams(rng, V, T), random_grams(rng, V, T, scale=0.1)
    bad[1, 1, 2, 5] = bad[1, 1, 5, 2] = np.nan            # object 1 only: a much better trial, but for the NaN
    dev = Device(rows, V, T, cq)
    first = dev(good, True)
    got = dev(bad, False)
    S = got["state"]
    assert S[:, tw.LAST_ACCEPT].tolist() == [1.0, 0.0, 1.0] and S[1, tw.REJECTED] == 1.0 and S[1, tw.STATUS] == tw.RUNNING
    assert S[1, tw.LAMBDA] == first["state"][1, tw.LAMBDA] * tw.DEFAULTS["lambda_up"]
    assert got["cur"][1].tobytes() == first["cur"][1].tobytes() and got["gram"][1].tobytes() == first["gram"][1].tobytes()
    assert np.isfinite(got["trial"]).all() and np.isfinite(got["cur"]).all() and np.isfinite(got["gram"]).all()
    # on init: no usable system for that object, its rows are the start; the others go on
    got = Device(rows, V, T, cq)(bad, True)
    assert got["state"][:, tw.STATUS].tolist() == [tw.RUNNING, tw.NO_SYSTEM, tw.RUNNING]
    assert got["trial"][1].tobytes() == got["cur"][1].tobytes() == rows[1].tobytes()
    assert np.isfinite(got["trial"]).all() and np.isfinite(got["cur"]).all()
