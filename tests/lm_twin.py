"""numpy float64 twin of ``sdfr_lm_step`` (test-side only): one Levenberg-Marquardt bookkeeping-and-solve step of K
estimates from their per-view Gram matrices, rule for rule as include/sdfr.h group 18 states it -- the mean cost, the
accept test, the damping floor, the freeze, "a rounded trial equal to the current row means converged".  It needs no
renderer: the Gram matrices are its input.  Nothing here imports the product.

What the kernel and the twin decide ALIKE (accept / reject, the status, lambda) rests on the cost, which both form with
the same IEEE operations in the same order: the view sums and |z|^2 are Python loops here, not ``np.sum`` (pairwise
from 8 terms on).  The normal equations, the solve and the retraction agree to rounding only."""
import numpy as np

from information_twin import qmul, tangent_map

# include/sdfr.h, group 18 (tests/test_lm_cpu.py holds them against the header)
STATE_DOUBLES = 16
(LAMBDA, COST, COUNT, STATUS, ACCEPTED, REJECTED, STEP_NORM, PREDICTED, ACTUAL, COST_INIT, COUNT_INIT, LAST_ACCEPT,
 COST_TRIAL, COUNT_TRIAL) = range(14)
RUNNING, CONVERGED, STALLED, NO_SYSTEM = range(4)
FLOOR = 1e-12

# the constants of a step, by the C entry's argument names (sdfest_amd.lm.LM_DEFAULTS holds the product's copy)
DEFAULTS = dict(latent_weight=0.0, min_overlap=0.5, lambda0=1e-3, lambda_up=10.0, lambda_down=0.1, lambda_min=1e-9,
                lambda_max=1e9, step_tol=1e-9)


def sums(gram, T):
    """(rss, cnt) of one object's (V,F,F) Gram matrices, views ascending"""
    rss = cnt = 0.0
    for G in gram:
        rss = rss + float(G[8 + T, 8 + T])
        cnt = cnt + float(G[9 + T, 9 + T])
    return rss, cnt


def cost(gram, row, T, mu):
    """(Phi, cnt): Phi = rss / cnt + mu |z|^2, NaN where a Gram entry or one of the row's first 8 + T entries is not
    finite or cnt is not positive"""
    rss, cnt = sums(gram, T)
    if not (np.isfinite(gram).all() and np.isfinite(np.asarray(row[:8 + T], np.float64)).all() and cnt > 0.0):
        return float("nan"), cnt
    zz = 0.0
    for j in range(T):
        z = float(row[8 + j])
        zz = zz + z * z
    with np.errstate(all="ignore"):
        return float(np.float64(rss) / np.float64(cnt) + np.float64(mu) * np.float64(zz)), cnt


def view_map(row, cam_quat_v, T):
    """M (8+T, 7+T) of one view: ``tangent_map`` at the camera-frame quaternion and 1 / scale, the identity on the latent"""
    row = np.asarray(row, np.float64)
    cq = np.asarray(cam_quat_v, np.float64)
    cq = cq / np.linalg.norm(cq)
    q = row[3:7] / np.linalg.norm(row[3:7])
    q_c = qmul(cq * np.array([-1.0, -1.0, -1.0, 1.0]), q)
    M = np.zeros((8 + T, 7 + T))
    M[:8, :7] = tangent_map(q_c, 1.0 / row[7], cq)
    M[8:, 7:] = np.eye(T)
    return M


def normal_equations(gram, row, cam_quat, T, mu):
    """(H, g): H = sum_v M^T G_v[:8+T,:8+T] M / cnt + mu I_latent, g = sum_v M^T G_v[:8+T,8+T] / cnt + mu z"""
    n, m = 7 + T, 8 + T
    H, g = np.zeros((n, n)), np.zeros(n)
    for G, cq in zip(np.asarray(gram, np.float64), cam_quat):
        M = view_map(row, cq, T)
        H += M.T @ G[:m, :m] @ M
        g += M.T @ G[:m, m]
    _, cnt = sums(gram, T)
    H, g = H / cnt, g / cnt
    H[7:, 7:] += mu * np.eye(T)
    g[7:] += mu * np.asarray(row[8:m], np.float64)
    return H, g


def damped(H, lam):
    """A = H + lambda diag(max(H_ii, FLOOR max_j H_jj))"""
    d = np.diag(H)
    return H + lam * np.diag(np.maximum(d, FLOOR * d.max()))


def retract(row, delta, T):
    """the first 8 + T entries of the row moved by the tangent step, float64 (the caller rounds)"""
    row = np.asarray(row, np.float64)
    out = row[:8 + T].copy()
    out[0:3] = row[0:3] + delta[0:3]
    w = delta[3:6]
    th = np.sqrt(w @ w)
    sh, ch = (np.sin(0.5 * th) / th, np.cos(0.5 * th)) if th > 1e-12 else (0.5, 1.0)
    q = qmul(np.append(w * sh, ch), row[3:7] / np.linalg.norm(row[3:7]))
    out[3:7] = q / np.linalg.norm(q)
    with np.errstate(over="ignore"):
        out[7] = row[7] * np.exp(delta[6])
    out[8:] = row[8:8 + T] + delta[7:]
    return out


def lm_step(gram_trial, params_trial, params_cur, gram_cur, state, cam_quat, T, init, row_dtype=np.float32,
            **constants):
    """One step for K objects.  gram_trial / gram_cur (K,V,F,F) float64, params_* (K,n_params), state (K,16),
    cam_quat (V,4).  Returns new (params_trial, params_cur, gram_cur, state, step (K,7+T), system) and changes no input;
    ``system[k]`` is (A, g) of the solve of row k, or None.  ``row_dtype``: the format the rows are rounded to -- the
    kernel's float32, or float64 to see the step without the parameter row's rounding."""
    c = dict(DEFAULTS, **constants)
    mu = float(c["latent_weight"])
    gt = np.asarray(gram_trial, np.float64)
    K = gt.shape[0]
    pt, pc = np.array(params_trial, row_dtype), np.array(params_cur, row_dtype)
    gc, S = np.array(gram_cur, np.float64), np.array(state, np.float64)
    n, m = 7 + T, 8 + T
    step, system = np.zeros((K, n)), [None] * K
    for k in range(K):
        if not init and S[k, STATUS] != 0.0:   # frozen
            pt[k] = pc[k]
            continue
        phi_t, cnt_t = cost(gt[k], pt[k], T, mu)
        status = RUNNING
        if init:
            accept, lam = True, float(c["lambda0"])
            phi_c, cnt_c, phi0, cnt0 = phi_t, cnt_t, phi_t, cnt_t
            n_acc = n_rej = norm = pred = actual = 0.0
        else:
            lam, phi_c, cnt_c, n_acc, n_rej, norm, pred, phi0, cnt0 = (
                S[k, i] for i in (LAMBDA, COST, COUNT, ACCEPTED, REJECTED, STEP_NORM, PREDICTED, COST_INIT, COUNT_INIT))
            accept = bool(np.isfinite(phi_t) and cnt_t >= c["min_overlap"] * cnt_c and phi_t < phi_c)
            actual = phi_c - phi_t if np.isfinite(phi_t) else float("nan")
            if accept:
                phi_c, cnt_c = phi_t, cnt_t
                lam = max(lam * c["lambda_down"], c["lambda_min"])
                n_acc += 1.0
                if norm < c["step_tol"]:
                    status = CONVERGED
            else:
                lam = lam * c["lambda_up"]
                n_rej += 1.0
                if lam > c["lambda_max"]:
                    status = STALLED
        if accept:
            pc[k], gc[k] = pt[k], gt[k]
        if status == RUNNING and not np.isfinite(phi_c):
            status = NO_SYSTEM
        if status == RUNNING:
            status = NO_SYSTEM
            with np.errstate(all="ignore"):
                H, g = normal_equations(gc[k], pc[k], cam_quat, T, mu)
                d = np.diag(H)
                if np.isfinite(H).all() and d.max() > 0.0:
                    A = damped(H, lam)
                    try:
                        Lc = np.linalg.cholesky(A)
                        delta = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
                    except np.linalg.LinAlgError:
                        delta = None
                    if delta is not None and np.isfinite(delta).all():
                        new = retract(pc[k], delta, T).astype(row_dtype)
                        new_norm = float(np.sqrt(np.sum(delta * delta * np.diag(A))))
                        new_pred = float(-(2.0 * g @ delta + delta @ H @ delta))
                        if np.isfinite(new).all() and np.isfinite(new_norm) and np.isfinite(new_pred):
                            norm, pred, step[k], system[k] = new_norm, new_pred, delta, (A, g)
                            status = RUNNING
                            if new.tobytes() == pc[k, :m].tobytes():
                                status = CONVERGED
                            else:
                                pt[k] = pc[k]
                                pt[k, :m] = new
        if status != RUNNING:
            pt[k] = pc[k]
        S[k] = 0.0
        S[k, :14] = (lam, phi_c, cnt_c, status, n_acc, n_rej, norm, pred, actual, phi0, cnt0, 1.0 if accept else 0.0,
                     phi_t, cnt_t)
    return pt, pc, gc, S, step, system


# ---- a test problem that needs no renderer ------------------------------------------------------------------------
def view_parameters(row, cam_quat_v, T):
    """what a view's Gram matrix differentiates by, as a function of the row: (camera-frame position for a camera at
    the origin, camera-frame unit quaternion, 1 / scale, latent) -- ``view_map`` is its Jacobian by the tangent step"""
    row = np.asarray(row, np.float64)
    cq = np.asarray(cam_quat_v, np.float64)
    cq = cq / np.linalg.norm(cq)
    x, y, z, w = cq
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    q_c = qmul(cq * np.array([-1.0, -1.0, -1.0, 1.0]), row[3:7] / np.linalg.norm(row[3:7]))
    return np.concatenate([R.T @ row[0:3], q_c, [1.0 / row[7]], row[8:8 + T]])


class LinearProblem:
    """Least squares posed as Gram matrices: per view a random J (pixels x (8+T)) and the residual
    r = J (view_parameters(row) - view_parameters(truth)), linear in what the Gram matrix differentiates by and zero at
    the truth.  ``gram(rows)`` is what the renderer's information call would hand to the step: (K,V,F,F) of f = (J, r, 1)."""

    def __init__(self, rng, T, V, pixels=200, latent=None):
        self.T, self.V = T, V
        self.n_params = 8 + (T if latent is None else latent)
        self.cam_quat = rng.standard_normal((V, 4))
        self.cam_quat /= np.linalg.norm(self.cam_quat, axis=1, keepdims=True)
        self.J = rng.standard_normal((V, pixels, 8 + T))
        q = rng.standard_normal(4)
        self.truth = np.concatenate([rng.uniform(-0.2, 0.2, 3) + [0.0, 0.0, -1.0], q / np.linalg.norm(q), [0.15],
                                     0.3 * rng.standard_normal(self.n_params - 8)])

    def start(self, rng, position=0.005, angle=np.radians(3.0), scale=0.02, latent=0.05):
        """the truth moved by `position` metres, `angle` radians, a relative `scale` and `latent` N(0, 1) per entry"""
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        d = rng.standard_normal(3)
        row = self.truth.copy()
        row[0:3] += position * d / np.linalg.norm(d)
        row[3:7] = qmul(np.append(axis * np.sin(0.5 * angle), np.cos(0.5 * angle)), self.truth[3:7])
        row[7] *= 1.0 + scale
        row[8:8 + self.T] += latent * rng.standard_normal(self.T)
        return row

    def gram(self, rows):
        rows = np.asarray(rows, np.float64).reshape(-1, self.n_params)
        T, F = self.T, 10 + self.T
        out = np.zeros((rows.shape[0], self.V, F, F))
        for k, row in enumerate(rows):
            for v in range(self.V):
                f = np.ones((self.J.shape[1], F))
                f[:, :8 + T] = self.J[v]
                f[:, 8 + T] = self.J[v] @ (view_parameters(row, self.cam_quat[v], T)
                                           - view_parameters(self.truth, self.cam_quat[v], T))
                out[k, v] = f.T @ f
        return out
