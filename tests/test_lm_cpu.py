"""CPU: ``sdfr_lm_step`` is declared, bound, exported and validates its arguments before any HIP call; the numpy twin
(tests/lm_twin.py) minimises a linear problem and handles the degenerate inputs the kernel is tested against on the
GPU (tests/test_lm_step_gpu.py)."""
import ctypes

import numpy as np
import pytest

import lm_twin as tw


@pytest.fixture(scope="module")
def L():
    from sdfest_amd import _lib
    _lib.build()
    return _lib.lib()


def test_lm_step_is_declared_bound_and_exported(L):
    from sdfest_amd import _lib
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert _lib.SIGNATURES["sdfr_lm_step"] == (i, [vp] * 7 + [i] * 5 + [d] * 8 + [i, vp])
    assert hasattr(L, "sdfr_lm_step")
    A = _lib.ABI
    assert A["SDFR_LM_STATE_DOUBLES"] == tw.STATE_DOUBLES
    names = ("LAMBDA", "COST", "COUNT", "STATUS", "ACCEPTED", "REJECTED", "STEP_NORM", "PREDICTED", "ACTUAL", "COST_INIT",
             "COUNT_INIT", "LAST_ACCEPT", "COST_TRIAL", "COUNT_TRIAL")
    assert [A["SDFR_LM_" + n] for n in names] == [getattr(tw, n) for n in names] == list(range(14))
    assert [A["SDFR_LM_" + n] for n in ("RUNNING", "CONVERGED", "STALLED", "NO_SYSTEM")] == [0, 1, 2, 3]
    # the product's constants are the twin's
    from sdfest_amd import lm
    assert dict(lm.LM_DEFAULTS, latent_weight=0.0, min_overlap=0.5) == tw.DEFAULTS
    import sdfest_amd
    assert sdfest_amd.lm_step is lm.lm_step and sdfest_amd.LMRefiner is lm.LMRefiner and sdfest_amd.LMReport is lm.LMReport


def test_lm_step_argument_errors_without_gpu(L):
    """every argument error comes back before any HIP call (the pointers are never dereferenced)"""
    from sdfest_amd import _lib
    INVALID, NULL = _lib.ABI["SDFR_E_INVALID"], _lib.ABI["SDFR_E_NULL"]
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: L.sdfr_last_error()
    good = dict(gram_trial=q, params_trial=q, params_cur=q, gram_cur=q, state=q, step=None, cam_quat=q, K=2, V=2, T=8,
                n_params=16, init=1, latent_weight=0.0, min_overlap=0.5, lambda0=1e-3, lambda_up=10.0, lambda_down=0.1,
                lambda_min=1e-9, lambda_max=1e9, step_tol=1e-9, device=0, stream=None)
    call = lambda **kw: L.sdfr_lm_step(*dict(good, **kw).values())
    for name in ("gram_trial", "params_trial", "params_cur", "gram_cur", "state", "cam_quat"):
        assert call(**{name: None}) == NULL and b"sdfr_lm_step" in err() and b"NULL" in err(), name
    for kw, msg in ((dict(T=23), b"T=23"), (dict(T=-1), b"T=-1"), (dict(V=65), b"V=65"), (dict(V=0), b"V=0"),
                    (dict(K=0), b"K=0"), (dict(K=65536), b"K=65536"), (dict(n_params=15), b"n_params=15"),
                    (dict(lambda0=-1e-3), b"lambda0"), (dict(lambda_max=float("inf")), b"lambda_max"),
                    (dict(step_tol=float("nan")), b"step_tol"), (dict(latent_weight=-1.0), b"latent_weight"),
                    (dict(min_overlap=float("nan")), b"min_overlap"),
                    (dict(state=ctypes.c_void_p(q.value + 4)), b"8-byte aligned"),
                    (dict(gram_cur=ctypes.c_void_p(q.value + 4)), b"8-byte aligned"),
                    (dict(step=ctypes.c_void_p(q.value + 4)), b"8-byte aligned")):
        assert call(**kw) == INVALID and b"sdfr_lm_step" in err() and msg in err(), (kw, err())


def _run(problem, rows, steps, row_dtype=np.float32, **constants):
    """the twin's iteration on a ``LinearProblem``: init, then `steps` further steps; yields every step's arrays"""
    T, K = problem.T, len(rows)
    pt = np.array(rows, row_dtype)
    pc, gc, S = np.zeros_like(pt), np.zeros((K, problem.V, 10 + T, 10 + T)), np.zeros((K, tw.STATE_DOUBLES))
    for it in range(steps + 1):
        judged = pt.copy()
        pt, pc, gc, S, step, system = tw.lm_step(problem.gram(pt), pt, pc, gc, S, problem.cam_quat, T, it == 0,
                                                 row_dtype=row_dtype, **constants)
        yield dict(judged=judged, trial=pt, cur=pc, gram=gc, state=S, step=step, system=system)


@pytest.mark.parametrize("T", [0, 1, 8, 22])
def test_twin_minimises_a_linear_problem(T):
    """r = J (parameters - truth) posed as Gram matrices, lambda0 = 1e-3: within 20 steps the gradient of the normal
    equations is below 1e-10 of its initial norm, and no accepted step raises Phi.  The rows are kept in float64 here:
    rounded to float32 the residual J (row - truth) cannot fall below ~6e-8 |J| |row|, which floors the gradient at
    1e-6 of the initial one for a start 5 % away -- the row's format, not the step's (the float32 run below has to
    reach THAT floor and stay monotone)."""
    rng = np.random.default_rng(100 + T)
    problem = tw.LinearProblem(rng, T, V=2)
    start = problem.start(rng)
    grad = lambda r: np.linalg.norm(tw.normal_equations(r["gram"][0], r["cur"][0], problem.cam_quat, T, 0.0)[1])
    costs, g0, g = [], None, None
    for r in _run(problem, [start], 20, row_dtype=np.float64, lambda0=1e-3):
        S = r["state"][0]
        g = grad(r)
        g0 = g if g0 is None else g0
        if S[tw.LAST_ACCEPT]:
            costs.append(S[tw.COST])
        assert S[tw.COST] == costs[-1]                      # a rejected trial leaves the current cost alone
        if S[tw.STATUS] != tw.RUNNING:                      # (frozen from here on)
            break
    print(f"T={T}: gradient {g0:.3e} -> {g:.3e} ({g / g0:.3e}), accepted costs {len(costs)}, Phi {costs[0]:.3e} -> {costs[-1]:.3e}")
    assert g <= 1e-10 * g0
    assert all(b < a for a, b in zip(costs, costs[1:]))
    # float32 rows, as the kernel keeps them: monotone, and down to the format's floor
    costs, g0 = [], None
    for r in _run(problem, [start], 20, lambda0=1e-3):
        S = r["state"][0]
        g = grad(r)
        g0 = g if g0 is None else g0
        if S[tw.LAST_ACCEPT]:
            costs.append(S[tw.COST])
        if S[tw.STATUS] != tw.RUNNING:
            break
    assert all(b < a for a, b in zip(costs, costs[1:])) and g <= 1e-4 * g0, (g / g0, costs)


def degenerate_zero_latent_column(rng):
    """(problem, rows): T = 8 with latent direction 3 unobserved -- its column of every J is zero"""
    problem = tw.LinearProblem(rng, 8, V=2)
    problem.J[:, :, 8 + 3] = 0.0
    return problem, [problem.start(rng)]


def test_twin_zero_latent_column_gives_a_zero_step_there():
    problem, rows = degenerate_zero_latent_column(np.random.default_rng(7))
    r = next(_run(problem, rows, 0, latent_weight=0.0))
    assert r["state"][0, tw.STATUS] == tw.RUNNING and np.isfinite(r["step"]).all()
    assert r["step"][0, 7 + 3] == 0.0 and np.abs(r["step"][0]).max() > 0.0
    assert r["trial"][0, 8 + 3] == r["cur"][0, 8 + 3] and np.isfinite(r["trial"]).all()


def test_twin_all_zero_gram_is_no_system():
    rng = np.random.default_rng(8)
    problem = tw.LinearProblem(rng, 8, V=2)
    rows = np.array([problem.start(rng)], np.float32)
    out = tw.lm_step(np.zeros((1, 2, 18, 18)), rows, np.zeros_like(rows), np.zeros((1, 2, 18, 18)), np.zeros((1, 16)),
                     problem.cam_quat, 8, True)
    assert out[3][0, tw.STATUS] == tw.NO_SYSTEM
    assert out[0].tobytes() == out[1].tobytes() == rows.tobytes()          # trial equals current equals the start


def test_twin_nan_in_a_trial_gram_is_rejected_or_no_system_on_init():
    rng = np.random.default_rng(9)
    problem = tw.LinearProblem(rng, 1, V=2)
    steps = _run(problem, [problem.start(rng)], 1)
    first = next(steps)
    bad = problem.gram(first["trial"])
    bad[0, 1, 2, 5] = bad[0, 1, 5, 2] = np.nan
    # on a later step: a reject, lambda grows, the current iterate stays, the new trial is finite
    pt, pc, gc, S, _, _ = tw.lm_step(bad, first["trial"], first["cur"], first["gram"], first["state"], problem.cam_quat, 1,
                                     False)
    assert S[0, tw.LAST_ACCEPT] == 0.0 and S[0, tw.REJECTED] == 1.0 and S[0, tw.STATUS] == tw.RUNNING
    assert S[0, tw.LAMBDA] == first["state"][0, tw.LAMBDA] * tw.DEFAULTS["lambda_up"]
    assert pc.tobytes() == first["cur"].tobytes() and gc.tobytes() == first["gram"].tobytes()
    assert np.isfinite(pt).all() and np.isfinite(pc).all()
    # on init: no usable system, and the rows are the start
    rows = first["judged"]
    pt, pc, gc, S, _, _ = tw.lm_step(bad, rows, np.zeros_like(rows), np.zeros_like(bad), np.zeros((1, 16)),
                                     problem.cam_quat, 1, True)
    assert S[0, tw.STATUS] == tw.NO_SYSTEM and pt.tobytes() == pc.tobytes() == rows.tobytes()
