// lm.hip -- sdfr_lm_step (gfx950 only): the bookkeeping-and-solve half of a Levenberg-Marquardt iteration over pose and
// latent, from the Gram matrices sdfr_render_information[_shape] writes (include/sdfr.h group 18).
//
// One workgroup per object, one wave per workgroup.  The work is a chain of small dependent steps -- judge the trial,
// copy it, project V Gram matrices of at most 32 x 32 into the 7 + T <= 29 tangent dimensions, one Cholesky
// factorisation, two triangular solves, one retraction --, none of which has work for more than a wave: the kernel is
// bound by the latency of that chain (LDS round trips, fp64 divisions and square roots), not by throughput, and K objects
// occupy K compute units.  The matrix cores have nothing to do here (fp64 MFMA blocks start at 16 x 16 x 4 and the
// factorisation is a sequence of 29 dependent columns).
//
// Everything is double.  What a float64 restatement has to decide ALIKE -- the cost and the accept test -- is written
// without contraction and in one stated order (lm_cost, the view sums); what it has to match to rounding only -- the
// normal equations, the solve, the retraction -- is free to fuse.  Every sum has one order and nothing is shared between
// workgroups: the same bits on every call, and row k does not depend on the launch's other rows.
#include <cmath>

#include "common.hpp"

namespace sdfr {
namespace {

constexpr int kLmMaxN = 7 + SDFR_INFO_MAX_TANGENTS;   // tangent dimensions
constexpr int kLmMaxM = 8 + SDFR_INFO_MAX_TANGENTS;   // parameters the Gram matrix differentiates by = entries of a moved row
constexpr double kLmFloor = 1e-12;      // damping floor relative to the largest diagonal entry (a condition, sdfr.h)

struct LmConstants {
  double mu, min_overlap, lambda0, up, down, lambda_min, lambda_max, step_tol;
};

// Phi = rss / cnt + mu |z|^2: IEEE operations in this order, no fused multiply-add -- numpy float64 gives the same bits
__device__ __forceinline__ double lm_cost(double rss, double cnt, double mu, const float* __restrict__ row, int T) {
#pragma clang fp contract(off)
  double zz = 0.0;
  for (int j = 0; j < T; ++j) {
    const double z = (double)row[8 + j];
    zz = zz + z * z;
  }
  return rss / cnt + mu * zz;
}

// uncertainty.tangent_map's T8 (8 x 7, row-major) at the unit camera-frame quaternion qc, inv_scale isc and the camera's
// world orientation cq (unit): identity | 1/2 (e_k, 0) (x) qc | -isc, position and rotation columns through R_c^T
__device__ __forceinline__ void lm_tangent_map(const double (&qc)[4], double isc, const double (&cq)[4], double (&t8)[56]) {
  const double x = cq[0], y = cq[1], z = cq[2], w = cq[3];
  // R_c row-major; M = R_c^T maps a world step to the camera frame: M[r][c] = rc[c][r]
  const double rc[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)},
                           {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)},
                           {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}};
  // column c of b: 1/2 (e_c, 0) (x) qc
  const double bx = qc[0], by = qc[1], bz = qc[2], bw = qc[3];
  const double b[4][3] = {{0.5 * bw, 0.5 * bz, -0.5 * by},
                          {-0.5 * bz, 0.5 * bw, 0.5 * bx},
                          {0.5 * by, -0.5 * bx, 0.5 * bw},
                          {-0.5 * bx, -0.5 * by, -0.5 * bz}};
#pragma unroll
  for (int i = 0; i < 56; ++i) t8[i] = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int j = 0; j < 3; ++j) t8[a * 7 + j] = rc[j][a];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      t8[(3 + a) * 7 + 3 + j] = b[a][0] * rc[j][0] + b[a][1] * rc[j][1] + b[a][2] * rc[j][2];
  t8[7 * 7 + 6] = -isc;
}

__device__ __forceinline__ void lm_quat_mul(const double (&a)[4], const double (&b)[4], double (&o)[4]) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
  o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}

// grid: K workgroups of one wave
__global__ __launch_bounds__(64) void lm_step_kernel(const double* gram_trial, float* params_trial, float* params_cur,
                                                     double* gram_cur, double* state, double* step,
                                                     const float* __restrict__ cam_quat, int V, int T, int np, int init,
                                                     LmConstants c) {
  __shared__ double sH[kLmMaxN * kLmMaxN];   // the normal matrix
  __shared__ double sA[kLmMaxN * kLmMaxN];   // the damped matrix, then its Cholesky factor (lower triangle)
  __shared__ double sg[kLmMaxN], sdiag[kLmMaxN], sx[kLmMaxN], stmp[kLmMaxN];
  __shared__ double sT8[56];
  __shared__ double sW[kLmMaxM * 7 + 7];     // G[:m][:8] T8, then (J^T r)[:8] T8
  __shared__ double srow[kLmMaxM], snew[kLmMaxM];
  __shared__ float scur[kLmMaxM];
  const int k = blockIdx.x, lane = threadIdx.x;
  const int F = 10 + T, n = 7 + T, m = 8 + T;
  const size_t FF = (size_t)F * F, gsz = (size_t)V * FF;
  const double* Gt = gram_trial + (size_t)k * gsz;
  double* Gc = gram_cur + (size_t)k * gsz;
  float* pt = params_trial + (size_t)k * np;
  float* pc = params_cur + (size_t)k * np;
  double* S = state + (size_t)k * SDFR_LM_STATE_DOUBLES;
  double* dl = step ? step + (size_t)k * n : nullptr;
  const double nan = __builtin_nan("");

  if (dl)
    for (int i = lane; i < n; i += 64) dl[i] = 0.0;
  if (!init && S[SDFR_LM_STATUS] != 0.0) {   // frozen: the trial is the current row, nothing else is touched
    for (int j = lane; j < np; j += 64) pt[j] = pc[j];
    return;
  }

  // ---- the trial's cost
  int fin = 1;
  for (size_t e = lane; e < gsz; e += 64) fin &= isfinite(Gt[e]) ? 1 : 0;
  for (int j = lane; j < m; j += 64) fin &= isfinite(pt[j]) ? 1 : 0;
  fin = __all(fin);
  double rss_t = 0.0, cnt_t = 0.0;
  for (int v = 0; v < V; ++v) {   // views ascending (additions only: nothing to contract)
    rss_t += Gt[v * FF + (size_t)(8 + T) * F + 8 + T];
    cnt_t += Gt[v * FF + (size_t)(9 + T) * F + 9 + T];
  }
  const double phi_t = (fin && cnt_t > 0.0) ? lm_cost(rss_t, cnt_t, c.mu, pt, T) : nan;

  // ---- accept or reject
  double lambda, phi_c, cnt_c, n_acc, n_rej, step_norm, pred, actual, phi0, cnt0;
  bool accept;
  int status = SDFR_LM_RUNNING;
  if (init) {
    accept = true;
    lambda = c.lambda0;
    phi_c = phi_t; cnt_c = cnt_t; phi0 = phi_t; cnt0 = cnt_t;
    n_acc = n_rej = step_norm = pred = actual = 0.0;
  } else {
    lambda = S[SDFR_LM_LAMBDA]; phi_c = S[SDFR_LM_COST]; cnt_c = S[SDFR_LM_COUNT];
    n_acc = S[SDFR_LM_ACCEPTED]; n_rej = S[SDFR_LM_REJECTED]; step_norm = S[SDFR_LM_STEP_NORM];
    pred = S[SDFR_LM_PREDICTED]; phi0 = S[SDFR_LM_COST_INIT]; cnt0 = S[SDFR_LM_COUNT_INIT];
    accept = isfinite(phi_t) && cnt_t >= c.min_overlap * cnt_c && phi_t < phi_c;   // (one product, no sum to fuse it into)
    actual = isfinite(phi_t) ? phi_c - phi_t : nan;
    if (accept) {
      phi_c = phi_t; cnt_c = cnt_t;
      lambda = fmax(lambda * c.down, c.lambda_min);
      n_acc += 1.0;
      if (step_norm < c.step_tol) status = SDFR_LM_CONVERGED;
    } else {
      lambda = lambda * c.up;
      n_rej += 1.0;
      if (lambda > c.lambda_max) status = SDFR_LM_STALLED;
    }
  }
  // the iterate the system is formed at: the trial where it was accepted (its copy below holds the same numbers)
  const double* G0 = accept ? Gt : Gc;
  const float* row0 = accept ? pt : pc;
  if (status == SDFR_LM_RUNNING && !isfinite(phi_c)) status = SDFR_LM_NO_SYSTEM;   // (init only: cnt = 0, a NaN)
  for (int j = lane; j < m; j += 64) {
    scur[j] = row0[j];
    srow[j] = (double)row0[j];
  }
  if (accept) {
    for (int j = lane; j < np; j += 64) pc[j] = pt[j];
    for (size_t e = lane; e < gsz; e += 64) Gc[e] = Gt[e];
  }
  __syncthreads();

  bool solved = false;
  if (status == SDFR_LM_RUNNING) {
    // ---- H = sum_v M^T G_v M / cnt + mu I_z,  g = sum_v M^T (J^T r)_v / cnt + mu z
    for (int e = lane; e < n * n; e += 64) sH[e] = 0.0;
    if (lane < n) sg[lane] = 0.0;
    const double qn = sqrt(srow[3] * srow[3] + srow[4] * srow[4] + srow[5] * srow[5] + srow[6] * srow[6]);
    const double q[4] = {srow[3] / qn, srow[4] / qn, srow[5] / qn, srow[6] / qn};
    const double isc = 1.0 / srow[7];
    for (int v = 0; v < V; ++v) {
      const double* G = G0 + v * FF;
      {
        double cq[4] = {(double)cam_quat[4 * v], (double)cam_quat[4 * v + 1], (double)cam_quat[4 * v + 2],
                        (double)cam_quat[4 * v + 3]};
        const double cn = sqrt(cq[0] * cq[0] + cq[1] * cq[1] + cq[2] * cq[2] + cq[3] * cq[3]);
        cq[0] /= cn; cq[1] /= cn; cq[2] /= cn; cq[3] /= cn;
        const double w2c[4] = {-cq[0], -cq[1], -cq[2], cq[3]};
        double qc[4], t8[56];
        lm_quat_mul(w2c, q, qc);
        const double qcn = sqrt(qc[0] * qc[0] + qc[1] * qc[1] + qc[2] * qc[2] + qc[3] * qc[3]);
        qc[0] /= qcn; qc[1] /= qcn; qc[2] /= qcn; qc[3] /= qcn;
        lm_tangent_map(qc, isc, cq, t8);
        if (lane == 0) {
#pragma unroll
          for (int i = 0; i < 56; ++i) sT8[i] = t8[i];
        }
      }
      __syncthreads();
      for (int e = lane; e < m * 7 + 7; e += 64) {
        const int a = e / 7, j = e - a * 7;
        double s = 0.0;
        if (a < m) {   // W[a][j] = sum_b G[a][b] T8[b][j]
          for (int b = 0; b < 8; ++b) s += G[(size_t)a * F + b] * sT8[b * 7 + j];
        } else {       // (J^T r)[:8] through T8
          for (int b = 0; b < 8; ++b) s += G[(size_t)b * F + m] * sT8[b * 7 + j];
        }
        sW[e] = s;
      }
      __syncthreads();
      for (int e = lane; e < n * n; e += 64) {
        const int i = e / n, j = e - i * n;
        const int hi = i > j ? i : j, lo = i > j ? j : i;   // the lower triangle's formula for both halves: H is symmetric
        double t;
        if (hi < 7) {
          t = 0.0;
          for (int a = 0; a < 8; ++a) t += sT8[a * 7 + hi] * sW[a * 7 + lo];
        } else if (lo < 7) {
          t = sW[(hi + 1) * 7 + lo];
        } else {
          t = G[(size_t)(hi + 1) * F + lo + 1];
        }
        sH[e] += t;
      }
      if (lane < n) sg[lane] += lane < 7 ? sW[m * 7 + lane] : G[(size_t)(lane + 1) * F + m];
      __syncthreads();
    }
    for (int e = lane; e < n * n; e += 64) {
      const int i = e / n, j = e - i * n;
      sH[e] = sH[e] / cnt_c + (i == j && i >= 7 ? c.mu : 0.0);
    }
    if (lane < n) sg[lane] = sg[lane] / cnt_c + (lane >= 7 ? c.mu * srow[lane + 1] : 0.0);
    __syncthreads();

    // ---- A = H + lambda diag(max(H_ii, floor max_j H_jj))
    double maxd = 0.0;
    for (int j = 0; j < n; ++j) maxd = fmax(maxd, sH[j * n + j]);
    bool ok = maxd > 0.0 && isfinite(maxd);
    for (int e = lane; e < n * n; e += 64) {
      const int i = e / n, j = e - i * n;
      double a = sH[e];
      if (i == j) {
        a += lambda * fmax(a, kLmFloor * maxd);
        sdiag[i] = a;
      }
      sA[e] = a;
    }
    __syncthreads();

    // ---- Cholesky, lane i owns row i: column j is A[i][j] - sum_{k<j} L[i][k] L[j][k], the pivot is lane j's
    for (int j = 0; ok && j < n; ++j) {
      double s = 0.0;
      if (lane >= j && lane < n) {
        s = sA[lane * n + j];
        for (int kk = 0; kk < j; ++kk) s -= sA[lane * n + kk] * sA[j * n + kk];
      }
      const double d = __shfl(s, j, 64);
      if (!(d > 0.0) || !isfinite(d)) {
        ok = false;   // (the same for every lane)
        break;
      }
      const double r = sqrt(d);
      if (lane >= j && lane < n) sA[lane * n + j] = lane == j ? r : s / r;
      __syncthreads();
    }
    if (ok) {
      // ---- L y = -g, L^T x = y
      double acc = 0.0, yv = 0.0, xv = 0.0;
      for (int j = 0; j < n; ++j) {
        const double cand = lane == j ? (-sg[j] - acc) / sA[j * n + j] : 0.0;
        const double yj = __shfl(cand, j, 64);
        if (lane == j) yv = yj;
        if (lane > j && lane < n) acc += sA[lane * n + j] * yj;
      }
      acc = 0.0;
      for (int j = n - 1; j >= 0; --j) {
        const double cand = lane == j ? (yv - acc) / sA[j * n + j] : 0.0;
        const double xj = __shfl(cand, j, 64);
        if (lane == j) xv = xj;
        if (lane < j) acc += sA[j * n + lane] * xj;
      }
      if (lane < n) sx[lane] = xv;
      __syncthreads();
      if (lane < n) {
        double hx = 0.0;
        for (int j = 0; j < n; ++j) hx += sH[lane * n + j] * sx[j];
        stmp[lane] = xv * hx;
      }
      __syncthreads();
      double nrm = 0.0, gx = 0.0, xhx = 0.0;
      for (int i = 0; i < n; ++i) {   // ascending, every lane the same
        nrm += sx[i] * sx[i] * sdiag[i];
        gx += sg[i] * sx[i];
        xhx += stmp[i];
      }
      const double new_norm = sqrt(nrm), new_pred = -(2.0 * gx + xhx);
      // ---- retraction (lane 0 states the pose part, lanes j < T the latent)
      if (lane == 0) {
        const double wx = sx[3], wy = sx[4], wz = sx[5];
        const double th = sqrt(wx * wx + wy * wy + wz * wz);
        double sh = 0.5, ch = 1.0;   // sin(th / 2) / th, cos(th / 2); th -> 0: the first terms of both series
        if (th > 1e-12) {
          sh = sin(0.5 * th) / th;
          ch = cos(0.5 * th);
        }
        const double dq[4] = {wx * sh, wy * sh, wz * sh, ch};
        double qq[4];
        lm_quat_mul(dq, q, qq);
        const double nn = sqrt(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3]);
        snew[0] = srow[0] + sx[0]; snew[1] = srow[1] + sx[1]; snew[2] = srow[2] + sx[2];
        snew[3] = qq[0] / nn; snew[4] = qq[1] / nn; snew[5] = qq[2] / nn; snew[6] = qq[3] / nn;
        snew[7] = srow[7] * exp(sx[6]);
      }
      if (lane < T) snew[8 + lane] = srow[8 + lane] + sx[7 + lane];
      __syncthreads();
      int finite = 1, same = 1;
      float mine = 0.0f;
      if (lane < m) {
        mine = (float)snew[lane];
        finite = isfinite(mine) ? 1 : 0;
        same = __float_as_uint(mine) == __float_as_uint(scur[lane]) ? 1 : 0;
      }
      finite = __all(finite) && isfinite(new_norm) && isfinite(new_pred);
      same = __all(same);
      if (!finite) {
        status = SDFR_LM_NO_SYSTEM;
      } else {
        solved = true;
        step_norm = new_norm;
        pred = new_pred;
        if (dl && lane < n) dl[lane] = sx[lane];
        if (same) status = SDFR_LM_CONVERGED;
        else if (lane < m) pt[lane] = mine;
      }
    } else {
      status = SDFR_LM_NO_SYSTEM;
    }
  }
  // the rest of the trial row is the current row's; a row that froze in this call has its current row as its trial
  const int from = solved && status == SDFR_LM_RUNNING ? m : 0;
  if (!accept)   // (an accepted trial's row IS the current row wherever the step did not write)
    for (int j = from + lane; j < np; j += 64) pt[j] = pc[j];

  if (lane == 0) {
    S[SDFR_LM_LAMBDA] = lambda;
    S[SDFR_LM_COST] = phi_c;
    S[SDFR_LM_COUNT] = cnt_c;
    S[SDFR_LM_STATUS] = (double)status;
    S[SDFR_LM_ACCEPTED] = n_acc;
    S[SDFR_LM_REJECTED] = n_rej;
    S[SDFR_LM_STEP_NORM] = step_norm;
    S[SDFR_LM_PREDICTED] = pred;
    S[SDFR_LM_ACTUAL] = actual;
    S[SDFR_LM_COST_INIT] = phi0;
    S[SDFR_LM_COUNT_INIT] = cnt0;
    S[SDFR_LM_LAST_ACCEPT] = accept ? 1.0 : 0.0;
    S[SDFR_LM_COST_TRIAL] = phi_t;
    S[SDFR_LM_COUNT_TRIAL] = cnt_t;
    S[14] = 0.0;
    S[15] = 0.0;
  }
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" int sdfr_lm_step(const double* gram_trial, float* params_trial, float* params_cur, double* gram_cur,
                            double* state, double* step, const float* cam_quat, int K, int V, int T, int n_params,
                            int init, double latent_weight, double min_overlap, double lambda0, double lambda_up,
                            double lambda_down, double lambda_min, double lambda_max, double step_tol, int device,
                            void* stream) {
  const char* fn = "sdfr_lm_step";
  if (K < 1 || K > 65535 || V < 1 || V > SDFR_LM_MAX_VIEWS || T < 0 || T > SDFR_INFO_MAX_TANGENTS || n_params < 8 + T ||
      n_params > 65535)
    return fail(SDFR_E_INVALID, "%s: K=%d, V=%d, T=%d, n_params=%d: need 1 <= K <= 65535, 1 <= V <= %d, 0 <= T <= %d, "
                "8 + T <= n_params <= 65535", fn, K, V, T, n_params, SDFR_LM_MAX_VIEWS, SDFR_INFO_MAX_TANGENTS);
  if (!gram_trial || !params_trial || !params_cur || !gram_cur || !state || !cam_quat)
    return fail(SDFR_E_NULL, "%s: NULL pointer argument", fn);
  if (((uintptr_t)gram_trial & 7u) || ((uintptr_t)gram_cur & 7u) || ((uintptr_t)state & 7u) || ((uintptr_t)step & 7u))
    return fail(SDFR_E_INVALID, "%s: gram_trial, gram_cur, state and step must be 8-byte aligned", fn);
  const double scalars[8] = {latent_weight, min_overlap, lambda0, lambda_up, lambda_down, lambda_min, lambda_max, step_tol};
  const char* names[8] = {"latent_weight", "min_overlap", "lambda0", "lambda_up", "lambda_down", "lambda_min",
                          "lambda_max", "step_tol"};
  for (int i = 0; i < 8; ++i)
    if (!(scalars[i] >= 0.0) || !std::isfinite(scalars[i]))
      return fail(SDFR_E_INVALID, "%s: %s=%g must be finite and >= 0", fn, names[i], scalars[i]);
  SDFR_HIP_TRY(hipSetDevice(device));
  const LmConstants c{latent_weight, min_overlap, lambda0, lambda_up, lambda_down, lambda_min, lambda_max, step_tol};
  hipLaunchKernelGGL(lm_step_kernel, dim3((unsigned)K), dim3(64), 0, (hipStream_t)stream, gram_trial, params_trial,
                     params_cur, gram_cur, state, step, cam_quat, V, T, n_params, init, c);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
