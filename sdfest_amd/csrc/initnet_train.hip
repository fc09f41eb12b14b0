// initnet_train.hip -- one training iteration of the single-shot initialisation network (include/sdfr.h group 11):
// VanillaPointNet + SDFPoseHead under train(), the four-term loss, the gradient of every parameter.
//   sdfest/initialization/pointnet.py:62-96            Linear -> BatchNorm1d (batch statistics) -> ReLU per point,
//                                                      dense links (set maximum concatenated), residual links, set max
//   sdfest/initialization/sdf_pose_network.py:88-115   the head on the N set features
//   sdfest/initialization/scripts/train.py:211-287     mse of latent / position / scale + orientation term
// Not a translation of the torch graph:
//   * the per-point layers, their data gradient and their weight gradient are GEMMs over the N M rows in exact fp32 on
//     the matrix cores (v_mfma_f32_16x16x4_f32); a dense link's concatenation never exists: the broadcast half of the
//     weight times the per-sample maximum is a per-sample bias [N][cout], and its gradient is the per-sample column sum
//     of dU;
//   * everything that is a sum over rows has one owner and a fixed order: a workgroup per (sample, 64 columns) walks
//     the sample's M rows in order and leaves one fp64 record, a second kernel adds the N records in order; the weight
//     gradient's K = N M is split over row blocks of kSplitRows whose 64 x 64 records are added in order.  No float
//     atomics, no integer atomics either: the first maximum of a set is found by the workgroup that owns the column.
#include "common.hpp"

#include <algorithm>
#include <vector>

struct sdfr_pose_trainer {
  struct Layer {
    int cin_f = 0, cin_g = 0, cout = 0;   // per-point inputs, broadcast inputs (a dense link), outputs
    int res = 0;                          // 0: none; 1: out = prev + out, prev = [F | G] split as out is (or no G at all);
                                          // 2: the last layer of a dense net as wide as [F | G] together
    int last = 0, out_g = 0;              // out_g: this layer's maximum is concatenated for the next one
    size_t w = 0, b = 0, gamma = 0, beta = 0;   // offsets into the flat parameter buffer
    size_t stat = 0;                      // running mean at stat, running variance at stat + cout
  };
  int device = 0, in_size = 0, bn = 0, dense = 0, residual = 0, head_bn = 0, latent = 0, cells = 0, n_out = 0;
  std::vector<Layer> bb, hd;
  Layer fin;
  size_t n_params = 0, n_stats = 0;
  int max_bb = 0, max_inner = 0, max_hd = 0;   // widest backbone layer, widest stored backbone layer, widest head row
  size_t max_wrec = 0;                          // largest cout * cin_f of the backbone
};

namespace sdfr {
namespace {

typedef sdfr_pose_trainer::Layer Layer;
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kT = 64, kLd = kT + 1;     // GEMM tile; LDS row stride (a multiple of 32 would put a wave's rows in one bank)
constexpr int kSplitRows = 1024;         // rows of one weight-gradient record
constexpr double kBnEps = 1e-5, kBnMomentum = 0.1;   // torch.nn.BatchNorm1d defaults
constexpr int kMaxWidth = 1 << 16;
// rows a thread of the per-sample passes loads before it uses any of them: with 32 x 2 workgroups on a narrow layer a
// CU holds a wave or two, and one load in flight per thread leaves the pass at 0.1 TB/s (the order of the sums stays)
constexpr int kRowBatch = 8;

// ---- the GEMMs ---------------------------------------------------------------------------------------------------------
// out[r][j] = sum_k X[r][k] B(j, k) + cvec[r / M][j] + resid[r][j],  B(j, k) = w[j * sj + k * sk];  out, cvec, resid
// have J columns.  Forward: B = the weight's rows (sj = ldw, sk = 1); data gradient: B = its columns (sj = 1, sk = ldw).
// grid (ceil(R / 64), ceil(J / 64)); a wave = 16 rows x 64 columns (4 accumulator tiles).
__global__ __launch_bounds__(256) void train_gemm_rows_kernel(const float* __restrict__ X, int R, int K, int ldx,
                                                              const float* __restrict__ w, long long sj, long long sk,
                                                              int J, const float* __restrict__ cvec, int M,
                                                              const float* __restrict__ resid, float* __restrict__ out) {
  __shared__ float xs[kT * kLd];
  __shared__ float ws[kT * kLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = lane & 15, kq = lane >> 4;
  const int p0 = blockIdx.x * kT, c0 = blockIdx.y * kT;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int kc = 0; kc < K; kc += kT) {
    const int kn = min(kT, K - kc);
    if (kc) __syncthreads();
    for (int i = tid; i < kT * kT; i += 256) {
      const int hi = i >> 6, lo = i & 63;
      xs[hi * kLd + lo] = (p0 + hi < R && lo < kn) ? X[(size_t)(p0 + hi) * ldx + kc + lo] : 0.0f;
      const int j = sk == 1 ? hi : lo, k = sk == 1 ? lo : hi;     // the unit stride goes to consecutive threads
      ws[j * kLd + k] = (c0 + j < J && k < kn) ? w[(size_t)(c0 + j) * sj + (size_t)(kc + k) * sk] : 0.0f;
    }
    __syncthreads();
    const int kp = (kn + 3) & ~3;
    for (int k0 = 0; k0 < kp; k0 += 4) {
      const float a = xs[(wave * 16 + row) * kLd + k0 + kq];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ws[(j * 16 + row) * kLd + k0 + kq], acc[j], 0, 0, 0);
    }
  }
  // the accumulator holds D[row 4 * kq + r][column `row`] of each tile
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = c0 + j * 16 + row;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = p0 + wave * 16 + kq * 4 + r;
      if (p < R && col < J) {
        float v = acc[j][r];
        if (cvec) v += cvec[(size_t)(p / M) * J + col];
        if (resid) v += resid[(size_t)p * J + col];
        out[(size_t)p * J + col] = v;
      }
    }
  }
}

// rec[s][c][k] = sum over the rows r of split s of dU[r][c] F[r][k]   (dU [R][C], F [R][Fw]);
// grid (splits, ceil(C / 64), ceil(Fw / 64)); a wave = 16 c x 64 k; the rows are the MFMA's reduction dimension.
__global__ __launch_bounds__(256) void train_wgrad_kernel(const float* __restrict__ dU, int C, const float* __restrict__ F,
                                                          int Fw, int R, float* __restrict__ rec) {
  __shared__ float as[kT * kLd];
  __shared__ float bs[kT * kLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = lane & 15, kq = lane >> 4;
  const int s = blockIdx.x, c0 = blockIdx.y * kT, k0 = blockIdx.z * kT;
  const int r_begin = s * kSplitRows, r_end = min(R, r_begin + kSplitRows);
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int rc = r_begin; rc < r_end; rc += kT) {
    if (rc != r_begin) __syncthreads();
    for (int i = tid; i < kT * kT; i += 256) {
      const int rr = i >> 6, lo = i & 63;
      const bool rok = rc + rr < r_end;
      as[rr * kLd + lo] = (rok && c0 + lo < C) ? dU[(size_t)(rc + rr) * C + c0 + lo] : 0.0f;
      bs[rr * kLd + lo] = (rok && k0 + lo < Fw) ? F[(size_t)(rc + rr) * Fw + k0 + lo] : 0.0f;
    }
    __syncthreads();
    for (int q = 0; q < kT; q += 4) {
      const float a = as[(q + kq) * kLd + wave * 16 + row];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bs[(q + kq) * kLd + j * 16 + row], acc[j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = k0 + j * 16 + row;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + wave * 16 + kq * 4 + r;
      if (c < C && k < Fw) rec[((size_t)s * C + c) * Fw + k] = acc[j][r];
    }
  }
}

// dW[c][k] = the records of the splits in order (fp64);  grid: ceil(C * Fw / 256)
__global__ void train_wgrad_combine_kernel(const float* __restrict__ rec, int splits, int C, int Fw, float* __restrict__ dw,
                                           int ldw) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)C * Fw;
  if (i >= n) return;
  double acc = 0.0;
  for (int s = 0; s < splits; ++s) acc += (double)rec[(size_t)s * n + i];
  dw[(i / Fw) * (size_t)ldw + i % Fw] = (float)acc;
}

// ---- passes over the rows of one sample: grid (N, ceil(C / 64)), 256 threads = 4 row groups x 64 columns -------------
// cst [4][C]: batch mean, 1 / sigma, gamma / sigma, beta (nullptr: no BatchNorm)
struct BnCol {
  float mean, invstd, scale, beta;
  bool on;
  __device__ __forceinline__ float z(float u) const { return on ? fmaf(u - mean, scale, beta) : u; }
  __device__ __forceinline__ float xhat(float u) const { return (u - mean) * invstd; }
};
__device__ __forceinline__ BnCol bn_col(const float* __restrict__ cst, int C, int c, bool ok) {
  BnCol b{0.0f, 1.0f, 1.0f, 0.0f, cst != nullptr};
  if (cst && ok) { b.mean = cst[c]; b.invstd = cst[C + c]; b.scale = cst[2 * C + c]; b.beta = cst[3 * C + c]; }
  return b;
}
__device__ __forceinline__ double group_sum(double v, double (*red)[64], int rg, int cl) {
  red[rg][cl] = v;
  __syncthreads();
  const double s = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
  __syncthreads();
  return s;
}

// rec[n][c] = sum_r U (mean == nullptr) or sum_r (U - mean[c])^2: the centred second pass of the batch variance
__global__ __launch_bounds__(256) void train_set_moment_kernel(const float* __restrict__ U, int M, int C,
                                                               const double* __restrict__ mean, double* __restrict__ rec) {
  __shared__ double red[4][64];
  const int n = blockIdx.x, cl = threadIdx.x & 63, rg = threadIdx.x >> 6, c = blockIdx.y * 64 + cl;
  const bool ok = c < C;
  const double mu = (mean && ok) ? mean[c] : 0.0;
  double acc = 0.0;
  if (ok)
    for (int r0 = rg; r0 < M; r0 += 4 * kRowBatch) {
      float u[kRowBatch];
#pragma unroll
      for (int i = 0; i < kRowBatch; ++i) u[i] = r0 + 4 * i < M ? U[((size_t)n * M + r0 + 4 * i) * C + c] : 0.0f;
#pragma unroll
      for (int i = 0; i < kRowBatch; ++i)
        if (r0 + 4 * i < M) {
          const double d = (double)u[i] - mu;
          acc += mean ? d * d : d;
        }
    }
  const double s = group_sum(acc, red, rg, cl);
  if (ok && rg == 0) rec[(size_t)n * C + c] = s;
}

// mean[c] = sum_n rec[n][c] / rows   (the N records in order);  grid ceil(C / 256)
__global__ void train_mean_kernel(const double* __restrict__ rec, int N, int C, double rows, double* __restrict__ mean) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int n = 0; n < N; ++n) s += rec[(size_t)n * C + c];
  mean[c] = s / rows;
}

// the batch statistics of one BatchNorm: cst, and the running statistics when `running` is given
__global__ void train_bn_finish_kernel(const double* __restrict__ rec, int N, int C, double rows,
                                       const double* __restrict__ mean, const float* __restrict__ gamma,
                                       const float* __restrict__ beta, float* __restrict__ cst,
                                       float* __restrict__ running) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int n = 0; n < N; ++n) s += rec[(size_t)n * C + c];
  const double var = s / rows, invstd = 1.0 / sqrt(var + kBnEps);
  cst[c] = (float)mean[c];
  cst[C + c] = (float)invstd;
  cst[2 * C + c] = (float)((double)gamma[c] * invstd);
  cst[3 * C + c] = beta[c];
  if (running) {
    running[c] = (float)((1.0 - kBnMomentum) * (double)running[c] + kBnMomentum * mean[c]);
    running[C + c] = (float)((1.0 - kBnMomentum) * (double)running[C + c] + kBnMomentum * (s / (rows - 1.0)));
  }
}

// what a residual link adds at (row, c): prev_out = [Fp | Gp broadcast]
__device__ __forceinline__ float resid_at(const float* __restrict__ Fp, int Fw, const float* __restrict__ Gp, int Gw,
                                          size_t row, int n, int c) {
  return c < Fw ? Fp[row * Fw + c] : Gp[(size_t)n * Gw + (c - Fw)];
}

// A = relu(bn(U)); out = A + residual -> Fout (nullable); the set maximum and its FIRST row of `out` (pool_out) or of A:
// pmax[n][c] (+ Gadd[n][c], the broadcast half a residual adds to a dense link's maximum), arg[n][c] in [0, M)
__global__ __launch_bounds__(256) void train_act_pool_kernel(const float* __restrict__ U, int M, int C,
                                                             const float* __restrict__ cst, const float* __restrict__ Fp,
                                                             int Fw, const float* __restrict__ Gp, int Gw,
                                                             float* __restrict__ Fout, int pool_out,
                                                             const float* __restrict__ Gadd, float* __restrict__ pmax,
                                                             int* __restrict__ arg) {
  __shared__ float bv[4][64];
  __shared__ int bi[4][64];
  const int n = blockIdx.x, cl = threadIdx.x & 63, rg = threadIdx.x >> 6, c = blockIdx.y * 64 + cl;
  const bool ok = c < C;
  const BnCol b = bn_col(cst, C, c, ok);
  float best = -INFINITY;
  int idx = 0;
  if (ok)
    for (int r0 = rg; r0 < M; r0 += 4 * kRowBatch) {
      float u[kRowBatch], res[kRowBatch];
#pragma unroll
      for (int i = 0; i < kRowBatch; ++i) {
        const int r = r0 + 4 * i;
        const size_t row = (size_t)n * M + r;
        u[i] = r < M ? U[row * C + c] : 0.0f;
        res[i] = (r < M && Fp) ? resid_at(Fp, Fw, Gp, Gw, row, n, c) : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < kRowBatch; ++i) {
        const int r = r0 + 4 * i;
        if (r < M) {
          const float a = fmaxf(b.z(u[i]), 0.0f);
          const float o = Fp ? a + res[i] : a;
          if (Fout) Fout[((size_t)n * M + r) * C + c] = o;
          const float pv = pool_out ? o : a;
          if (pv > best) { best = pv; idx = r; }     // rows ascend: the first maximum of this group
        }
      }
    }
  bv[rg][cl] = best;
  bi[rg][cl] = idx;
  __syncthreads();
  if (ok && rg == 0 && pmax) {
    for (int g = 1; g < 4; ++g) {
      const float v = bv[g][cl];
      const int i = bi[g][cl];
      if (v > best || (v == best && i < idx)) { best = v; idx = i; }
    }
    pmax[(size_t)n * C + c] = Gadd ? best + Gadd[(size_t)n * C + c] : best;
    arg[(size_t)n * C + c] = idx;
  }
}

// d loss / d Z at (row, c): the dense gradient gF (nullable) plus what the set maximum routes to its row, behind ReLU
// gP: the gradient of the set maximum, fp32 (a dense link's) or fp64 (gPd: the last layer's, which the head's backward
// leaves in fp64 -- see train_head_act_bwd_kernel)
struct DzSrc {
  const float* U; const float* gF; const int* arg; const float* gP; const double* gPd;
};
// what a thread of column c of sample n keeps for its walk: the maximum's row (-1: none) and its gradient
struct DzCol { int arg; double gp; };
__device__ __forceinline__ DzCol dz_col(const DzSrc& s, int C, int n, int c, bool ok) {
  DzCol d{-1, 0.0};
  if (ok && s.arg) {
    d.arg = s.arg[(size_t)n * C + c];
    d.gp = s.gPd ? s.gPd[(size_t)n * C + c] : (double)s.gP[(size_t)n * C + c];
  }
  return d;
}
__device__ __forceinline__ double dz_of(const BnCol& b, const DzCol& d, int r, float u, float gf) {
  if (!(b.z(u) > 0.0f)) return 0.0;
  double g = (double)gf;
  if (d.arg == r) g += d.gp;
  return g;
}
// the rows r0, r0 + 4, ... of a batch: U and the dense gradient, loaded before any of them is used
__device__ __forceinline__ void dz_load(const DzSrc& s, int M, int C, int n, int r0, int c, float* u, float* gf) {
#pragma unroll
  for (int i = 0; i < kRowBatch; ++i) {
    const int r = r0 + 4 * i;
    const size_t at = ((size_t)n * M + r) * C + c;
    u[i] = r < M ? s.U[at] : 0.0f;
    gf[i] = (r < M && s.gF) ? s.gF[at] : 0.0f;
  }
}

// the two column sums of the BatchNorm backward: rec1[n][c] = sum_r dZ, rec2[n][c] = sum_r dZ xhat
__global__ __launch_bounds__(256) void train_bn_bwd_sums_kernel(DzSrc src, int M, int C, const float* __restrict__ cst,
                                                                double* __restrict__ rec1, double* __restrict__ rec2) {
  __shared__ double red[4][64];
  const int n = blockIdx.x, cl = threadIdx.x & 63, rg = threadIdx.x >> 6, c = blockIdx.y * 64 + cl;
  const bool ok = c < C;
  const BnCol b = bn_col(cst, C, c, ok);
  const DzCol dc = dz_col(src, C, n, c, ok);
  double a1 = 0.0, a2 = 0.0;
  if (ok)
    for (int r0 = rg; r0 < M; r0 += 4 * kRowBatch) {
      float u[kRowBatch], gf[kRowBatch];
      dz_load(src, M, C, n, r0, c, u, gf);
#pragma unroll
      for (int i = 0; i < kRowBatch; ++i)
        if (r0 + 4 * i < M) {
          const double dz = dz_of(b, dc, r0 + 4 * i, u[i], gf[i]);
          a1 += dz;
          a2 += dz * (double)b.xhat(u[i]);
        }
    }
  const double s1 = group_sum(a1, red, rg, cl), s2 = group_sum(a2, red, rg, cl);
  if (ok && rg == 0) { rec1[(size_t)n * C + c] = s1; rec2[(size_t)n * C + c] = s2; }
}

// d beta = sum dZ, d gamma = sum dZ xhat (the N records in order), and their means for the dU pass
__global__ void train_bn_bwd_finish_kernel(const double* __restrict__ rec1, const double* __restrict__ rec2, int N, int C,
                                           double rows, float* __restrict__ d_gamma, float* __restrict__ d_beta,
                                           float* __restrict__ bst) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int n = 0; n < N; ++n) { s1 += rec1[(size_t)n * C + c]; s2 += rec2[(size_t)n * C + c]; }
  d_beta[c] = (float)s1;
  d_gamma[c] = (float)s2;
  bst[c] = (float)(s1 / rows);
  bst[C + c] = (float)(s2 / rows);
}

// dU = gamma / sigma (dZ - mean dZ - xhat mean(dZ xhat)) (or dZ without BatchNorm) -> dU [R][C], and its per-sample
// column sum S[n][c]: the bias gradient and the dense link's gradient are sums of S
__global__ __launch_bounds__(256) void train_du_kernel(DzSrc src, int M, int C, const float* __restrict__ cst,
                                                       const float* __restrict__ bst, float* __restrict__ dU,
                                                       float* __restrict__ S) {
  __shared__ double red[4][64];
  const int n = blockIdx.x, cl = threadIdx.x & 63, rg = threadIdx.x >> 6, c = blockIdx.y * 64 + cl;
  const bool ok = c < C;
  const BnCol b = bn_col(cst, C, c, ok);
  const float m1 = (cst && ok) ? bst[c] : 0.0f, m2 = (cst && ok) ? bst[C + c] : 0.0f;
  const DzCol dc = dz_col(src, C, n, c, ok);
  double acc = 0.0;
  if (ok)
    for (int r0 = rg; r0 < M; r0 += 4 * kRowBatch) {
      float u[kRowBatch], gf[kRowBatch];
      dz_load(src, M, C, n, r0, c, u, gf);
#pragma unroll
      for (int i = 0; i < kRowBatch; ++i) {
        const int r = r0 + 4 * i;
        if (r < M) {
          const float dz = (float)dz_of(b, dc, r, u[i], gf[i]);
          const float du = cst ? b.scale * (dz - m1 - b.xhat(u[i]) * m2) : dz;
          dU[((size_t)n * M + r) * C + c] = du;
          acc += (double)du;
        }
      }
    }
  const double s = group_sum(acc, red, rg, cl);
  if (ok && rg == 0) S[(size_t)n * C + c] = (float)s;
}

// ---- launch-sized kernels: N rows ---------------------------------------------------------------------------------------
// y[n][col] = W[col][koff .. koff + K) . x[n] + bias[col]; one wave per (n, col); grid ceil(N * C / 4)
__global__ __launch_bounds__(256) void train_rows_linear_kernel(const float* __restrict__ w, int ldw, int koff,
                                                                const float* __restrict__ x, int K,
                                                                const float* __restrict__ bias, float* __restrict__ y,
                                                                int N, int C) {
  const long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (o >= (long long)N * C) return;
  const int n = (int)(o / C), col = (int)(o % C);
  const float acc = wave_dot(x + (size_t)n * K, w + (size_t)col * ldw + koff, K, lane);
  if (lane == 0) y[o] = acc + bias[col];
}

// y[n][c] = bias[c] for every sample (the per-sample bias of a layer without a dense link)
__global__ void train_rows_bias_kernel(const float* __restrict__ bias, float* __restrict__ y, int N, int C) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)N * C) y[i] = bias[i % C];
}

// the head's BatchNorm (batch statistics over the N rows, one thread per column) and ReLU: H = relu(bn(U))
__global__ void train_head_act_kernel(const float* __restrict__ U, int N, int C, const float* __restrict__ gamma,
                                      const float* __restrict__ beta, float* __restrict__ cst, float* __restrict__ running,
                                      float* __restrict__ H) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  BnCol b{0.0f, 1.0f, 1.0f, 0.0f, gamma != nullptr};
  if (gamma) {
    double s = 0.0;
    for (int n = 0; n < N; ++n) s += (double)U[(size_t)n * C + c];
    const double mean = s / N;
    double v = 0.0;
    for (int n = 0; n < N; ++n) { const double d = (double)U[(size_t)n * C + c] - mean; v += d * d; }
    const double invstd = 1.0 / sqrt(v / N + kBnEps);
    b.mean = (float)mean; b.invstd = (float)invstd; b.scale = (float)((double)gamma[c] * invstd); b.beta = beta[c];
    cst[c] = b.mean; cst[C + c] = b.invstd; cst[2 * C + c] = b.scale; cst[3 * C + c] = b.beta;
    if (running) {
      running[c] = (float)((1.0 - kBnMomentum) * (double)running[c] + kBnMomentum * mean);
      running[C + c] = (float)((1.0 - kBnMomentum) * (double)running[C + c] + kBnMomentum * (v / (N - 1.0)));
    }
  }
  for (int n = 0; n < N; ++n) H[(size_t)n * C + c] = fmaxf(b.z(U[(size_t)n * C + c]), 0.0f);
}

// backward of the above: gH [N][C] -> dU [N][C] (in place allowed: a thread owns its column), d gamma, d beta.
// The head's gradient rows are fp64 from the final layer down to the set feature: the columns of a BatchNorm's dU sum to
// zero over the batch, and what reaches a backbone parameter whose only effect the head's first BatchNorm removes (the
// last backbone BatchNorm's bias of a channel whose maximum is positive in every sample) is that cancellation.  In fp32
// it leaves 1e-7 of the terms, which Adam's normalisation turns into steps of lr; in fp64 it stays below Adam's eps, as
// in the reference's arithmetic carried out exactly.  N rows: the cost is nothing.
__global__ void train_head_act_bwd_kernel(const float* __restrict__ U, int N, int C, const float* __restrict__ cst,
                                          const double* gH, double* dU, float* __restrict__ d_gamma,
                                          float* __restrict__ d_beta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const BnCol b = bn_col(cst, C, c, true);
  // the batch mean and 1 / sigma again, in fp64 (the tape holds them rounded to fp32: xhat would not sum to zero)
  double mean = 0.0, invstd = 1.0, scale = 1.0;
  if (cst) {
    for (int n = 0; n < N; ++n) mean += (double)U[(size_t)n * C + c];
    mean /= N;
    double v = 0.0;
    for (int n = 0; n < N; ++n) { const double d = (double)U[(size_t)n * C + c] - mean; v += d * d; }
    invstd = 1.0 / sqrt(v / N + kBnEps);
    scale = (double)b.scale / (double)b.invstd * invstd;     // gamma / sigma
  }
  double s1 = 0.0, s2 = 0.0;
  if (cst) {
    for (int n = 0; n < N; ++n) {
      const float u = U[(size_t)n * C + c];
      const double dz = b.z(u) > 0.0f ? gH[(size_t)n * C + c] : 0.0;
      s1 += dz;
      s2 += dz * (((double)u - mean) * invstd);
    }
    d_beta[c] = (float)s1;
    d_gamma[c] = (float)s2;
  }
  const double m1 = s1 / N, m2 = s2 / N;
  for (int n = 0; n < N; ++n) {
    const float u = U[(size_t)n * C + c];
    const double dz = b.z(u) > 0.0f ? gH[(size_t)n * C + c] : 0.0;
    dU[(size_t)n * C + c] = cst ? scale * (dz - m1 - (((double)u - mean) * invstd) * m2) : dz;
  }
}

// dW[c][koff + k] = sum_n D[n][c] X[n][k] (n in order); one thread per (c, k); grid ceil(C * K / 256)
template <typename T>   // (T: float, or double for the head's gradient rows)
__global__ void train_rows_wgrad_kernel(const T* __restrict__ D, const float* __restrict__ X, int N, int C, int K,
                                        float* __restrict__ dw, int ldw, int koff) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)C * K) return;
  const int c = (int)(i / K), k = (int)(i % K);
  double acc = 0.0;
  for (int n = 0; n < N; ++n) acc = fma((double)D[(size_t)n * C + c], (double)X[(size_t)n * K + k], acc);
  dw[(size_t)c * ldw + koff + k] = (float)acc;
}

// db[c] = sum_n D[n][c] (n in order, fp64)
template <typename T>
__global__ void train_rows_bgrad_kernel(const T* __restrict__ D, int N, int C, float* __restrict__ db) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double acc = 0.0;
  for (int n = 0; n < N; ++n) acc += (double)D[(size_t)n * C + c];
  db[c] = (float)acc;
}

// gX[n][k] = sum_c D[n][c] W[c][koff + k] + add[n][k] (c in order); one thread per (n, k)
template <typename TI, typename TO>
__global__ void train_rows_dgrad_kernel(const TI* __restrict__ D, const float* __restrict__ w, int ldw, int koff, int N,
                                        int C, int K, const TO* __restrict__ add, TO* __restrict__ gX) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)N * K) return;
  const int n = (int)(i / K), k = (int)(i % K);
  double acc = 0.0;
  for (int c = 0; c < C; ++c) acc = fma((double)D[(size_t)n * C + c], (double)w[(size_t)c * ldw + koff + k], acc);
  gX[i] = (TO)(add ? acc + (double)add[i] : acc);
}

// the residual link into the last layer: the set maximum's gradient also reaches prev_out = [F | G] at its row.  One
// thread per (n, c): every target element has one writer.
__global__ void train_last_resid_kernel(const double* __restrict__ gP, const int* __restrict__ arg, int N, int M, int C,
                                        int Fw, int Gw, float* __restrict__ gF, float* __restrict__ gG) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)N * C) return;
  const int n = (int)(i / C), c = (int)(i % C);
  if (c < Fw) {
    if (gF) gF[((size_t)n * M + arg[i]) * Fw + c] += (float)gP[i];
  } else if (gG) {
    gG[(size_t)n * Gw + (c - Fw)] += (float)gP[i];
  }
}

// ---- the loss ------------------------------------------------------------------------------------------------------------
// one wave per output row: rowrec[n][4] = the row's share of the four SUMS, g_out[n] = d total / d out[n]
__global__ __launch_bounds__(64) void train_loss_rows_kernel(const float* __restrict__ out, int N, int L, int cells,
                                                             const float* __restrict__ t_latent,
                                                             const float* __restrict__ t_position,
                                                             const float* __restrict__ t_scale,
                                                             const int* __restrict__ t_index,
                                                             const float* __restrict__ t_quat, float w_latent,
                                                             float w_position, float w_scale, float w_orientation,
                                                             double* __restrict__ rowrec, float* __restrict__ g_out) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int n_out = L + 4 + (cells ? cells : 4);
  const float* o = out + (size_t)n * n_out;
  float* g = g_out + (size_t)n * n_out;
  auto wave_sum = [](double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
  };
  double sl = 0.0;
  for (int k = lane; k < L; k += 64) {
    const float d = o[k] - t_latent[(size_t)n * L + k];
    sl += (double)d * (double)d;
    g[k] = w_latent * 2.0f * d / ((float)N * (float)L);
  }
  sl = wave_sum(sl);
  double sp = 0.0;
  if (lane < 3) {
    const float d = o[L + lane] - t_position[(size_t)n * 3 + lane];
    sp = (double)d * (double)d;
    g[L + lane] = w_position * 2.0f * d / ((float)N * 3.0f);
  }
  sp = wave_sum(sp);
  const float ds = o[L + 3] - t_scale[n];
  if (lane == 0) g[L + 3] = w_scale * 2.0f * ds / (float)N;
  double so;
  const float* q = o + L + 4;
  if (cells) {   // cross entropy of the logits against the class index
    float m = -INFINITY;
    for (int k = lane; k < cells; k += 64) m = fmaxf(m, q[k]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    double se = 0.0;
    for (int k = lane; k < cells; k += 64) se += (double)expf(q[k] - m);
    se = wave_sum(se);
    const int idx = t_index[n];
    const bool idx_ok = idx >= 0 && idx < cells;
    so = idx_ok ? log(se) + (double)m - (double)q[idx] : (double)NAN;
    const float inv = (float)(1.0 / se);
    for (int k = lane; k < cells; k += 64)
      g[L + 4 + k] = w_orientation / (float)N * (expf(q[k] - m) * inv - (k == idx ? 1.0f : 0.0f));
  } else {       // 1 - (q / |q| . t)^2, through the normalisation
    const float* t = t_quat + (size_t)n * 4;
    const float nn = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float u[4] = {q[0] / nn, q[1] / nn, q[2] / nn, q[3] / nn};
    const float d = u[0] * t[0] + u[1] * t[1] + u[2] * t[2] + u[3] * t[3];
    so = 1.0 - (double)d * (double)d;
    if (lane < 4) g[L + 4 + lane] = w_orientation / (float)N * (-2.0f * d) * (t[lane] - d * u[lane]) / nn;
  }
  if (lane == 0) {
    rowrec[(size_t)n * 4 + 0] = sl;
    rowrec[(size_t)n * 4 + 1] = sp;
    rowrec[(size_t)n * 4 + 2] = (double)ds * (double)ds;
    rowrec[(size_t)n * 4 + 3] = so;
  }
}

// terms[5] = {latent, position, scale, orientation, total}: the rows in order
__global__ void train_loss_finish_kernel(const double* __restrict__ rowrec, int N, int L, float w_latent, float w_position,
                                         float w_scale, float w_orientation, float* __restrict__ terms) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < 4; ++k) s[k] += rowrec[(size_t)n * 4 + k];
  const double t[4] = {s[0] / ((double)N * L), s[1] / ((double)N * 3.0), s[2] / N, s[3] / N};
  for (int k = 0; k < 4; ++k) terms[k] = (float)t[k];
  terms[4] = (float)((double)w_latent * t[0] + (double)w_position * t[1] + (double)w_scale * t[2] +
                     (double)w_orientation * t[3]);
}

// ---- host: layouts ---------------------------------------------------------------------------------------------------------
inline size_t up64(size_t n) { return (n + 63) & ~(size_t)63; }

struct LayerTape { size_t U, F, G, arg, cst; };
struct Tape {
  std::vector<LayerTape> bb, hd;   // head: U, F = H, cst
  size_t pooled = 0, total = 0;    // in floats
};
Tape tape_layout(const sdfr_pose_trainer* t, int N, int M) {
  Tape tp;
  size_t off = 0;
  const size_t R = (size_t)N * M;
  auto take = [&off](size_t n) { const size_t o = off; off += up64(n); return o; };
  for (const Layer& l : t->bb) {
    LayerTape lt{};
    lt.U = take(R * l.cout);
    lt.F = l.last ? 0 : take(R * l.cout);
    lt.G = l.out_g ? take((size_t)N * l.cout) : 0;
    lt.arg = (l.out_g || l.last) ? take((size_t)N * l.cout) : 0;
    lt.cst = t->bn ? take(4 * (size_t)l.cout) : 0;
    tp.bb.push_back(lt);
  }
  tp.pooled = take((size_t)N * t->bb.back().cout);
  for (const Layer& l : t->hd) {
    LayerTape lt{};
    lt.U = take((size_t)N * l.cout);
    lt.F = take((size_t)N * l.cout);
    lt.cst = t->head_bn ? take(4 * (size_t)l.cout) : 0;
    tp.hd.push_back(lt);
  }
  tp.total = off;
  return tp;
}

struct Work {   // offsets in floats; the fp64 regions start at even offsets of an 8-byte aligned buffer
  size_t rowrec, cvec, rec1, rec2, dmean, bst, dU, gF[2], gG[2], gP, S, wrec, hA, hB, total;
};
Work work_layout(const sdfr_pose_trainer* t, int N, int M) {
  Work w{};
  size_t off = 0;
  const size_t R = (size_t)N * M, nb = (size_t)N * t->max_bb;
  auto take = [&off](size_t n) { const size_t o = off; off += up64(n); return o; };
  const int splits = (int)((R + kSplitRows - 1) / kSplitRows);
  w.rowrec = take(2 * 4 * (size_t)N);   // first: the loss is not told M, and this offset does not depend on it
  w.cvec = take(nb);
  w.rec1 = take(2 * nb);
  w.rec2 = take(2 * nb);
  w.dmean = take(2 * (size_t)t->max_bb);
  w.bst = take(2 * (size_t)t->max_bb);
  w.dU = take(R * t->max_bb);
  w.gF[0] = take(R * t->max_inner);
  w.gF[1] = take(R * t->max_inner);
  w.gG[0] = take(nb);
  w.gG[1] = take(nb);
  w.gP = take(2 * nb);                        // fp64
  w.S = take(nb);
  w.wrec = take((size_t)splits * t->max_wrec);
  w.hA = take(2 * (size_t)N * t->max_hd);     // fp64
  w.hB = take(2 * (size_t)N * t->max_hd);
  w.total = off;
  return w;
}

inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }
inline dim3 set_grid(int N, int C) { return dim3((unsigned)N, (unsigned)((C + 63) / 64)); }

const char* check_shape(const sdfr_pose_trainer* t, int N, int M) {
  if (N < 1 || N > 65535) return "N out of range (1 .. 65535)";
  if (M < 1 || (long long)N * M > (1LL << 30)) return "M out of range (N M <= 2^30)";
  if (t->bn && (long long)N * M < 2) return "BatchNorm needs more than one row";
  if (t->head_bn && N < 2) return "the head's BatchNorm needs N >= 2";
  return nullptr;
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" int sdfr_pose_trainer_create(int in_size, int n_backbone, const int* backbone_out, int batchnorm, int dense,
                                        int residual, int n_head, const int* head_out, int head_batchnorm, int latent,
                                        int n_cells, int device, sdfr_pose_trainer** out_handle) {
  const char* fn = "sdfr_pose_trainer_create";
  if (!out_handle) return fail(SDFR_E_NULL, "%s: NULL out_handle", fn);
  *out_handle = nullptr;
  if (!backbone_out || !head_out) return fail(SDFR_E_NULL, "%s: NULL layer list", fn);
  if (in_size < 1 || in_size > kMaxWidth) return fail(SDFR_E_INVALID, "%s: in_size %d out of range", fn, in_size);
  if (n_backbone < 1 || n_backbone > 64) return fail(SDFR_E_INVALID, "%s: n_backbone %d out of range", fn, n_backbone);
  if (n_head < 1 || n_head > 64) return fail(SDFR_E_INVALID, "%s: n_head %d out of range", fn, n_head);
  if (latent < 1 || latent > kMaxWidth) return fail(SDFR_E_INVALID, "%s: latent %d out of range", fn, latent);
  if (n_cells < 0 || n_cells > kMaxWidth) return fail(SDFR_E_INVALID, "%s: n_cells %d out of range", fn, n_cells);
  for (int i = 0; i < n_backbone; ++i)
    if (backbone_out[i] < 1 || backbone_out[i] > kMaxWidth)
      return fail(SDFR_E_INVALID, "%s: backbone layer %d has width %d", fn, i, backbone_out[i]);
  for (int i = 0; i < n_head; ++i)
    if (head_out[i] < 1 || head_out[i] > kMaxWidth)
      return fail(SDFR_E_INVALID, "%s: head layer %d has width %d", fn, i, head_out[i]);
  sdfr_pose_trainer* t = new sdfr_pose_trainer;
  t->device = device; t->in_size = in_size; t->bn = batchnorm != 0; t->dense = dense != 0; t->residual = residual != 0;
  t->head_bn = head_batchnorm != 0; t->latent = latent; t->cells = n_cells;
  t->n_out = latent + 4 + (n_cells ? n_cells : 4);
  int fw = in_size, gw = 0;
  for (int i = 0; i < n_backbone; ++i) {
    Layer l;
    l.cin_f = fw; l.cin_g = gw; l.cout = backbone_out[i];
    l.last = i == n_backbone - 1;
    l.out_g = (t->dense && !l.last) ? 1 : 0;
    if (t->residual && fw + gw == l.cout * (l.out_g ? 2 : 1)) {   // prev_out.shape == out.shape (pointnet.py:88-90)
      if (fw == l.cout) l.res = 1;
      else if (l.last && gw > 0) l.res = 2;
      else {
        delete t;
        return fail(SDFR_E_INVALID, "%s: backbone layer %d: a residual link from %d inputs onto a dense link's %d + %d "
                    "outputs mixes per-point and broadcast columns (not implemented)", fn, i, fw, l.cout, l.cout);
      }
    }
    t->bb.push_back(l);
    fw = l.cout; gw = l.out_g ? l.cout : 0;
  }
  for (int i = 0; i < n_head; ++i) {
    Layer l;
    l.cin_f = fw; l.cout = head_out[i];
    t->hd.push_back(l);
    fw = l.cout;
  }
  t->fin.cin_f = fw; t->fin.cout = t->n_out;
  // parameters() order: module registration order, torch's layouts
  size_t off = 0, soff = 0;
  for (Layer& l : t->bb) { l.w = off; off += (size_t)l.cout * (l.cin_f + l.cin_g); l.b = off; off += l.cout; }
  if (t->bn) for (Layer& l : t->bb) { l.gamma = off; off += l.cout; l.beta = off; off += l.cout; l.stat = soff; soff += 2 * (size_t)l.cout; }
  for (Layer& l : t->hd) { l.w = off; off += (size_t)l.cout * l.cin_f; l.b = off; off += l.cout; }
  if (t->head_bn) for (Layer& l : t->hd) { l.gamma = off; off += l.cout; l.beta = off; off += l.cout; l.stat = soff; soff += 2 * (size_t)l.cout; }
  t->fin.w = off; off += (size_t)t->fin.cout * t->fin.cin_f; t->fin.b = off; off += t->fin.cout;
  t->n_params = off; t->n_stats = soff;
  for (const Layer& l : t->bb) {
    t->max_bb = std::max(t->max_bb, l.cout);
    if (!l.last) t->max_inner = std::max(t->max_inner, l.cout);
    t->max_wrec = std::max(t->max_wrec, (size_t)l.cout * l.cin_f);
  }
  t->max_inner = std::max(t->max_inner, 1);
  t->max_hd = std::max(t->n_out, t->bb.back().cout);
  for (const Layer& l : t->hd) t->max_hd = std::max(t->max_hd, l.cout);
  *out_handle = t;
  return 0;
}

extern "C" void sdfr_pose_trainer_destroy(sdfr_pose_trainer* t) { delete t; }
extern "C" size_t sdfr_pose_trainer_param_count(const sdfr_pose_trainer* t) { return t ? t->n_params : 0; }
extern "C" size_t sdfr_pose_trainer_stat_count(const sdfr_pose_trainer* t) { return t ? t->n_stats : 0; }
extern "C" int sdfr_pose_trainer_output_size(const sdfr_pose_trainer* t) { return t ? t->n_out : 0; }

extern "C" size_t sdfr_pose_trainer_tape_bytes(const sdfr_pose_trainer* t, int N, int M) {
  if (!t || check_shape(t, N, M)) return 0;
  return (tape_layout(t, N, M).total + 64) * sizeof(float);
}

extern "C" size_t sdfr_pose_trainer_workspace_bytes(const sdfr_pose_trainer* t, int N, int M) {
  if (!t || check_shape(t, N, M)) return 0;
  return (work_layout(t, N, M).total + 64) * sizeof(float);
}

extern "C" int sdfr_pose_trainer_forward(const sdfr_pose_trainer* t, const float* params, float* stats,
                                         const float* points, int N, int M, int update_stats, float* out, float* tape,
                                         size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "sdfr_pose_trainer_forward";
  if (!t) return fail(SDFR_E_NULL, "%s: NULL trainer", fn);
  if (const char* why = check_shape(t, N, M)) return fail(SDFR_E_INVALID, "%s: N=%d M=%d: %s", fn, N, M, why);
  if (!params || !points || !out || !tape || !workspace) return fail(SDFR_E_NULL, "%s: NULL pointer argument", fn);
  if (update_stats && t->n_stats && !stats) return fail(SDFR_E_NULL, "%s: update_stats without a statistics buffer", fn);
  if ((uintptr_t)workspace & 7) return fail(SDFR_E_INVALID, "%s: the workspace must be 8-byte aligned", fn);
  if (tape_bytes < sdfr_pose_trainer_tape_bytes(t, N, M))
    return fail(SDFR_E_WORKSPACE, "%s: tape %zu < %zu bytes", fn, tape_bytes, sdfr_pose_trainer_tape_bytes(t, N, M));
  if (workspace_bytes < sdfr_pose_trainer_workspace_bytes(t, N, M))
    return fail(SDFR_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes,
                sdfr_pose_trainer_workspace_bytes(t, N, M));
  SDFR_HIP_TRY(hipSetDevice(t->device));
  hipStream_t st = (hipStream_t)stream;
  const Tape tp = tape_layout(t, N, M);
  const Work wk = work_layout(t, N, M);
  float* ws = static_cast<float*>(workspace);
  float* cvec = ws + wk.cvec;
  double* rec = reinterpret_cast<double*>(ws + wk.rec1);
  double* dmean = reinterpret_cast<double*>(ws + wk.dmean);
  const int R = N * M;
  float* run = update_stats ? stats : nullptr;
  const float* Fp = points;     // prev_out = [Fp | Gp]
  const float* Gp = nullptr;
  for (size_t i = 0; i < t->bb.size(); ++i) {
    const Layer& l = t->bb[i];
    const LayerTape& lt = tp.bb[i];
    const int C = l.cout, ldw = l.cin_f + l.cin_g;
    float* U = tape + lt.U;
    float* cst = t->bn ? tape + lt.cst : nullptr;
    // the per-sample bias: b + W[:, cin_f:] . G[n]
    if (l.cin_g)
      hipLaunchKernelGGL(train_rows_linear_kernel, dim3(blocks((size_t)N * C * 64)), dim3(256), 0, st, params + l.w, ldw,
                         l.cin_f, Gp, l.cin_g, params + l.b, cvec, N, C);
    else
      hipLaunchKernelGGL(train_rows_bias_kernel, dim3(blocks((size_t)N * C)), dim3(256), 0, st, params + l.b, cvec, N, C);
    hipLaunchKernelGGL(train_gemm_rows_kernel, dim3((unsigned)((R + kT - 1) / kT), (unsigned)((C + kT - 1) / kT)), dim3(256),
                       0, st, Fp, R, l.cin_f, l.cin_f, params + l.w, (long long)ldw, 1LL, C, cvec, M,
                       (const float*)nullptr, U);
    if (t->bn) {
      hipLaunchKernelGGL(train_set_moment_kernel, set_grid(N, C), dim3(256), 0, st, U, M, C, (const double*)nullptr, rec);
      hipLaunchKernelGGL(train_mean_kernel, dim3(blocks(C)), dim3(256), 0, st, rec, N, C, (double)R, dmean);
      hipLaunchKernelGGL(train_set_moment_kernel, set_grid(N, C), dim3(256), 0, st, U, M, C, (const double*)dmean, rec);
      hipLaunchKernelGGL(train_bn_finish_kernel, dim3(blocks(C)), dim3(256), 0, st, rec, N, C, (double)R,
                         (const double*)dmean, params + l.gamma, params + l.beta, cst, run ? run + l.stat : nullptr);
    }
    float* Fout = l.last ? nullptr : tape + lt.F;
    float* pmax = l.last ? tape + tp.pooled : (l.out_g ? tape + lt.G : nullptr);
    int* arg = (l.last || l.out_g) ? reinterpret_cast<int*>(tape + lt.arg) : nullptr;
    hipLaunchKernelGGL(train_act_pool_kernel, set_grid(N, C), dim3(256), 0, st, U, M, C, cst, l.res ? Fp : nullptr,
                       l.cin_f, Gp, l.cin_g, Fout, l.last, (l.res == 1 && l.out_g && l.cin_g) ? Gp : nullptr, pmax, arg);
    Fp = Fout;
    Gp = l.out_g ? tape + lt.G : nullptr;
  }
  const float* x = tape + tp.pooled;
  for (size_t j = 0; j < t->hd.size(); ++j) {
    const Layer& l = t->hd[j];
    const LayerTape& lt = tp.hd[j];
    hipLaunchKernelGGL(train_rows_linear_kernel, dim3(blocks((size_t)N * l.cout * 64)), dim3(256), 0, st, params + l.w,
                       l.cin_f, 0, x, l.cin_f, params + l.b, tape + lt.U, N, l.cout);
    hipLaunchKernelGGL(train_head_act_kernel, dim3(blocks(l.cout)), dim3(256), 0, st, tape + lt.U, N, l.cout,
                       t->head_bn ? params + l.gamma : nullptr, t->head_bn ? params + l.beta : nullptr,
                       t->head_bn ? tape + lt.cst : nullptr, (run && t->head_bn) ? run + l.stat : nullptr, tape + lt.F);
    x = tape + lt.F;
  }
  hipLaunchKernelGGL(train_rows_linear_kernel, dim3(blocks((size_t)N * t->n_out * 64)), dim3(256), 0, st, params + t->fin.w,
                     t->fin.cin_f, 0, x, t->fin.cin_f, params + t->fin.b, out, N, t->n_out);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_pose_trainer_loss(const sdfr_pose_trainer* t, const float* out, const float* latent,
                                      const float* position, const float* scale, const int* orientation_index,
                                      const float* orientation_quat, int N, float w_latent, float w_position,
                                      float w_scale, float w_orientation, float* terms, float* g_out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  const char* fn = "sdfr_pose_trainer_loss";
  if (!t) return fail(SDFR_E_NULL, "%s: NULL trainer", fn);
  if (N < 1 || N > 65535) return fail(SDFR_E_INVALID, "%s: N=%d out of range", fn, N);
  if (!out || !latent || !position || !scale || !terms || !g_out || !workspace)
    return fail(SDFR_E_NULL, "%s: NULL pointer argument", fn);
  if (t->cells ? !orientation_index : !orientation_quat)
    return fail(SDFR_E_NULL, "%s: the orientation target (%s) is NULL", fn, t->cells ? "class index" : "quaternion");
  if ((uintptr_t)workspace & 7) return fail(SDFR_E_INVALID, "%s: the workspace must be 8-byte aligned", fn);
  const size_t need = sdfr_pose_trainer_workspace_bytes(t, N, 1);
  if (workspace_bytes < need) return fail(SDFR_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
  SDFR_HIP_TRY(hipSetDevice(t->device));
  hipStream_t st = (hipStream_t)stream;
  double* rowrec = reinterpret_cast<double*>(static_cast<float*>(workspace) + work_layout(t, N, 1).rowrec);
  hipLaunchKernelGGL(train_loss_rows_kernel, dim3((unsigned)N), dim3(64), 0, st, out, N, t->latent, t->cells, latent,
                     position, scale, orientation_index, orientation_quat, w_latent, w_position, w_scale, w_orientation,
                     rowrec, g_out);
  hipLaunchKernelGGL(train_loss_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)rowrec, N, t->latent, w_latent,
                     w_position, w_scale, w_orientation, terms);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_pose_trainer_backward(const sdfr_pose_trainer* t, const float* params, const float* points, int N,
                                          int M, const float* tape, const float* g_out, float* grads, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  const char* fn = "sdfr_pose_trainer_backward";
  if (!t) return fail(SDFR_E_NULL, "%s: NULL trainer", fn);
  if (const char* why = check_shape(t, N, M)) return fail(SDFR_E_INVALID, "%s: N=%d M=%d: %s", fn, N, M, why);
  if (!params || !points || !tape || !g_out || !grads || !workspace)
    return fail(SDFR_E_NULL, "%s: NULL pointer argument", fn);
  if ((uintptr_t)workspace & 7) return fail(SDFR_E_INVALID, "%s: the workspace must be 8-byte aligned", fn);
  if (workspace_bytes < sdfr_pose_trainer_workspace_bytes(t, N, M))
    return fail(SDFR_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes,
                sdfr_pose_trainer_workspace_bytes(t, N, M));
  SDFR_HIP_TRY(hipSetDevice(t->device));
  hipStream_t st = (hipStream_t)stream;
  const Tape tp = tape_layout(t, N, M);
  const Work wk = work_layout(t, N, M);
  float* ws = static_cast<float*>(workspace);
  const int R = N * M;
  // ---- the head, from the final layer down: gH = d total / d (the layer's output), fp64 rows
  const int nh = (int)t->hd.size();
  double* gH = reinterpret_cast<double*>(ws + wk.hA);
  double* other = reinterpret_cast<double*>(ws + wk.hB);
  double* gPd = reinterpret_cast<double*>(ws + wk.gP);
  {
    const float* x = tape + tp.hd[nh - 1].F;
    const Layer& f = t->fin;
    hipLaunchKernelGGL(train_rows_wgrad_kernel<float>, dim3(blocks((size_t)f.cout * f.cin_f)), dim3(256), 0, st, g_out, x,
                       N, f.cout, f.cin_f, grads + f.w, f.cin_f, 0);
    hipLaunchKernelGGL(train_rows_bgrad_kernel<float>, dim3(blocks(f.cout)), dim3(256), 0, st, g_out, N, f.cout,
                       grads + f.b);
    hipLaunchKernelGGL((train_rows_dgrad_kernel<float, double>), dim3(blocks((size_t)N * f.cin_f)), dim3(256), 0, st, g_out,
                       params + f.w, f.cin_f, 0, N, f.cout, f.cin_f, (const double*)nullptr, gH);
  }
  for (int j = nh - 1; j >= 0; --j) {
    const Layer& l = t->hd[j];
    const LayerTape& lt = tp.hd[j];
    const float* x = j ? tape + tp.hd[j - 1].F : tape + tp.pooled;
    // gH -> dU in place
    hipLaunchKernelGGL(train_head_act_bwd_kernel, dim3(blocks(l.cout)), dim3(256), 0, st, tape + lt.U, N, l.cout,
                       t->head_bn ? tape + lt.cst : nullptr, (const double*)gH, gH, t->head_bn ? grads + l.gamma : nullptr,
                       t->head_bn ? grads + l.beta : nullptr);
    hipLaunchKernelGGL(train_rows_wgrad_kernel<double>, dim3(blocks((size_t)l.cout * l.cin_f)), dim3(256), 0, st,
                       (const double*)gH, x, N, l.cout, l.cin_f, grads + l.w, l.cin_f, 0);
    hipLaunchKernelGGL(train_rows_bgrad_kernel<double>, dim3(blocks(l.cout)), dim3(256), 0, st, (const double*)gH, N, l.cout,
                       grads + l.b);
    double* gx = j ? other : gPd;
    hipLaunchKernelGGL((train_rows_dgrad_kernel<double, double>), dim3(blocks((size_t)N * l.cin_f)), dim3(256), 0, st,
                       (const double*)gH, params + l.w, l.cin_f, 0, N, l.cout, l.cin_f, (const double*)nullptr, gx);
    if (j) std::swap(gH, other);
  }
  // ---- the backbone, from the last layer down.  gF / gG: d total / d [F_i | G_i] of the layer being processed
  const float* gF = nullptr;
  const float* gG = nullptr;
  int cur = 0;
  double* rec1 = reinterpret_cast<double*>(ws + wk.rec1);
  double* rec2 = reinterpret_cast<double*>(ws + wk.rec2);
  float* bst = ws + wk.bst;
  float* dU = ws + wk.dU;
  float* S = ws + wk.S;
  for (int i = (int)t->bb.size() - 1; i >= 0; --i) {
    const Layer& l = t->bb[i];
    const LayerTape& lt = tp.bb[i];
    const int C = l.cout, ldw = l.cin_f + l.cin_g;
    const float* cst = t->bn ? tape + lt.cst : nullptr;
    const float* Fprev = i ? tape + tp.bb[i - 1].F : points;
    const float* Gprev = l.cin_g ? tape + tp.bb[i - 1].G : nullptr;
    DzSrc src{tape + lt.U, gF, (l.last || l.out_g) ? reinterpret_cast<const int*>(tape + lt.arg) : nullptr,
              l.last ? nullptr : gG, l.last ? gPd : nullptr};
    if (t->bn) {
      hipLaunchKernelGGL(train_bn_bwd_sums_kernel, set_grid(N, C), dim3(256), 0, st, src, M, C, cst, rec1, rec2);
      hipLaunchKernelGGL(train_bn_bwd_finish_kernel, dim3(blocks(C)), dim3(256), 0, st, (const double*)rec1,
                         (const double*)rec2, N, C, (double)R, grads + l.gamma, grads + l.beta, bst);
    }
    hipLaunchKernelGGL(train_du_kernel, set_grid(N, C), dim3(256), 0, st, src, M, C, cst, (const float*)bst, dU, S);
    // the weight's per-point columns: split over row blocks, the records added in order
    const int splits = (R + kSplitRows - 1) / kSplitRows;
    hipLaunchKernelGGL(train_wgrad_kernel,
                       dim3((unsigned)splits, (unsigned)((C + kT - 1) / kT), (unsigned)((l.cin_f + kT - 1) / kT)), dim3(256),
                       0, st, (const float*)dU, C, Fprev, l.cin_f, R, ws + wk.wrec);
    hipLaunchKernelGGL(train_wgrad_combine_kernel, dim3(blocks((size_t)C * l.cin_f)), dim3(256), 0, st,
                       (const float*)(ws + wk.wrec), splits, C, l.cin_f, grads + l.w, ldw);
    // its broadcast columns and the bias: sums of the per-sample column sums
    if (l.cin_g)
      hipLaunchKernelGGL(train_rows_wgrad_kernel<float>, dim3(blocks((size_t)C * l.cin_g)), dim3(256), 0, st, (const float*)S,
                         Gprev, N, C, l.cin_g, grads + l.w, ldw, l.cin_f);
    hipLaunchKernelGGL(train_rows_bgrad_kernel<float>, dim3(blocks(C)), dim3(256), 0, st, (const float*)S, N, C, grads + l.b);
    if (i == 0) break;    // (no gradient w.r.t. the points)
    float* gF_prev = ws + wk.gF[cur];
    float* gG_prev = l.cin_g ? ws + wk.gG[cur] : nullptr;
    cur ^= 1;
    hipLaunchKernelGGL(train_gemm_rows_kernel, dim3((unsigned)((R + kT - 1) / kT), (unsigned)((l.cin_f + kT - 1) / kT)),
                       dim3(256), 0, st, (const float*)dU, R, C, C, params + l.w, 1LL, (long long)ldw, l.cin_f,
                       (const float*)nullptr, M, (l.res == 1 && !l.last) ? gF : nullptr, gF_prev);
    if (l.cin_g)
      hipLaunchKernelGGL((train_rows_dgrad_kernel<float, float>), dim3(blocks((size_t)N * l.cin_g)), dim3(256), 0, st, (const float*)S,
                         params + l.w, ldw, l.cin_f, N, C, l.cin_g, (l.res == 1 && !l.last) ? gG : nullptr, gG_prev);
    if (l.last && l.res)
      hipLaunchKernelGGL(train_last_resid_kernel, dim3(blocks((size_t)N * C)), dim3(256), 0, st,
                         (const double*)gPd, reinterpret_cast<const int*>(tape + lt.arg), N, M, C, l.cin_f,
                         l.cin_g, gF_prev, gG_prev);
    gF = gF_prev;
    gG = gG_prev;
  }
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
