// initnet.hip -- forward of the single-shot initialisation network that starts the render-and-compare
// loop: VanillaPointNet backbone + SDFPoseHead, inference mode.
//   sdfest/initialization/pointnet.py:7-96          per-point MLP (Linear -> BatchNorm1d -> ReLU), optional
//                                                   dense links (the set maximum is concatenated to every
//                                                   point) and residual links, then max over the points
//   sdfest/initialization/sdf_pose_network.py:9-115 MLP on the set feature, final Linear ->
//                                                   (latent, position, scale, orientation)
//   sdfest/estimation/simple_setup.py:795-812       softmax of the orientation logits, optional prior
//                                                   adjustment (:978-1009), argmax
// Not a translation of the torch graph:
//   * the per-point layers are GEMMs (points x channels) on the matrix cores in exact fp32
//     (v_mfma_f32_16x16x4_f32), with bias, the folded BatchNorm, ReLU, the residual sum and the column
//     maximum over the set in the epilogue -- the (M, 2C) concatenation of a dense link never exists: its
//     second half is the same vector for every point, so W[:, C:] . max goes into the layer's bias;
//   * the last backbone layer (M x 1024) is never written: only its column maximum leaves the kernel.
// The per-point layer's tile is initnet_tile.hpp (the batched layer of initnet_eval.hip runs the same one); the head
// and the dense links' biases are one kernel, linear_rows_kernel, behind sdfr_linear_vec (one row) and
// sdfr_linear_rows (N rows).
#include "common.hpp"
#include "initnet_tile.hpp"

#include <algorithm>

namespace sdfr {
namespace {

// The per-point layer (pointnet_tile, initnet_tile.hpp) on ONE set: x [M][ldx], colmax[col] = max over the points.
// grid (row blocks, ceil(cout / 64)): row block b takes the row tiles b, b + gridDim.x, ...
__global__ __launch_bounds__(256) void pointnet_layer_kernel(
    const float* __restrict__ x, int M, int cin, int ldx, const float* __restrict__ w, int ldw,
    const float* __restrict__ cvec, const float* __restrict__ bn_scale, const float* __restrict__ bn_shift,
    const float* __restrict__ resid, float* __restrict__ y, int ldy, int cout, int* __restrict__ colmax,
    const int* __restrict__ row_count) {
  __shared__ float xs[kPtsPerBlock * kTileLd];
  __shared__ float ws[kColsPerBlock * kTileLd];
  __shared__ int wave_max[4][kColsPerBlock];
  // row_count (sdfr_pointnet_layer_counted): the number of points lives on the device and M is the buffers' capacity;
  // the grid's row blocks stride over the real rows (workgroup-uniform loop)
  if (row_count) M = min(max(row_count[0], 0), M);
  for (int p0 = blockIdx.x * kPtsPerBlock; p0 < M; p0 += gridDim.x * kPtsPerBlock) {
    if (p0 != (int)blockIdx.x * kPtsPerBlock) __syncthreads();   // (the previous tile's LDS reads are done)
    pointnet_tile<false, true>(xs, ws, wave_max, nullptr, x, M, p0, cin, ldx, w, ldw, cvec, bn_scale, bn_shift, resid, y,
                               ldy, cout, colmax);
  }
}

// o = a (x) b, quaternion_multiply (quaternion_utils.py:12-33), scalar last -- the camera -> world product of an
// orientation, shared by init_estimate_kernel and init_hypotheses_kernel so that both give the same bits.  Every
// component is  fma(+-a1, b., fma(a3, b., +-(a0 * b.))) +- (a2 * b.)  with each rounding spelled out: the form the
// compiler gave init_estimate_kernel's plain expression, pinned here so that it no longer depends on the surrounding
// code (tests/hypotheses_twin.py states the same four lines in numpy).
__device__ __forceinline__ void quat_mul_world(const float* a, const float* b, float* o) {
  o[0] = __fsub_rn(fmaf(a[1], b[2], fmaf(a[3], b[0], __fmul_rn(a[0], b[3]))), __fmul_rn(a[2], b[1]));
  o[1] = __fadd_rn(fmaf(a[1], b[3], fmaf(a[3], b[1], -__fmul_rn(a[0], b[2]))), __fmul_rn(a[2], b[0]));
  o[2] = __fadd_rn(fmaf(-a[1], b[0], fmaf(a[3], b[2], __fmul_rn(a[0], b[1]))), __fmul_rn(a[2], b[3]));
  o[3] = __fsub_rn(fmaf(-a[1], b[1], fmaf(a[3], b[3], -__fmul_rn(a[0], b[0]))), __fmul_rn(a[2], b[2]));
}

// simple_setup.py:790-838 for ONE view, on the device: the head's output row -> the estimate in the world frame,
// written straight into the loop's parameter vector [position 3 | orientation 4 | scale 1 | latent L].
//   head [L + 4 + C] (discretised: latent, position, scale, C orientation logits) or [L + 8] (quaternion)
//   grid_quats [C][4] + index (the argmax of sdfr_orientation_posterior): the orientation of the chosen cell
//   centroid (nullable): added to the position (`position += centroid`, :793-794)
//   cam_pos [3], cam_quat [4]: camera in the world (:819-825): p_w = q_c (p, 0) q_c* + t_c, q_w = q_c q
//   take_if_better: 0 = "first" (always written); 1 = "best": written only if post_max[0] > best[0], which it then
//   becomes (:835-838; best[0] starts at 0)
__global__ void init_estimate_kernel(const float* __restrict__ head, int L, const float* __restrict__ grid_quats,
                                     const int* __restrict__ index, const float* __restrict__ centroid,
                                     const float* __restrict__ cam_pos, const float* __restrict__ cam_quat,
                                     int mean_shape, int take_if_better, const float* __restrict__ post_max,
                                     float* __restrict__ best, float* __restrict__ params) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (take_if_better) {
    if (!(post_max[0] > best[0])) return;
    best[0] = post_max[0];
  }
  float p[3] = {head[L], head[L + 1], head[L + 2]};
  if (centroid) { p[0] += centroid[0]; p[1] += centroid[1]; p[2] += centroid[2]; }
  float q[4];
  if (grid_quats) {
    const int i = index[0];
    for (int k = 0; k < 4; ++k) q[k] = grid_quats[4 * i + k];
  } else {   // sdf_pose_network.py:97-101: the head normalises its quaternion
    const float* o = head + L + 4;
    const float n = sqrtf(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
    for (int k = 0; k < 4; ++k) q[k] = o[k] / n;
  }
  const float c[4] = {cam_quat[0], cam_quat[1], cam_quat[2], cam_quat[3]};
  // quaternion_multiply (quaternion_utils.py:12-33), scalar last
  auto mul = [](const float* a, const float* b, float* o) {
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  };
  const float pq[4] = {p[0], p[1], p[2], 0.0f}, ci[4] = {-c[0], -c[1], -c[2], c[3]};
  float t[4], r[4], qw[4];
  mul(c, pq, t);      // quaternion_apply (:36-54): q (p, 0) q^-1
  mul(t, ci, r);
  quat_mul_world(c, q, qw);
  params[0] = r[0] + cam_pos[0]; params[1] = r[1] + cam_pos[1]; params[2] = r[2] + cam_pos[2];
  for (int k = 0; k < 4; ++k) params[3 + k] = qw[k];
  params[7] = head[L + 3];
  for (int k = 0; k < L; ++k) params[8 + k] = mean_shape ? 0.0f : head[k];
}

// y[n][col] = act((W[col][koff .. koff + k) . x[n] + bias[col]) * s[col] + t[col]); one wave per (row n = blockIdx.y,
// column): the head and a dense link's per-set bias, for one set (sdfr_linear_vec) or N (sdfr_linear_rows)
__global__ __launch_bounds__(256) void linear_rows_kernel(const float* __restrict__ w, int ldw, int koff,
                                                          const float* __restrict__ x, int ldx, int k,
                                                          const float* __restrict__ bias,
                                                          const float* __restrict__ bn_scale,
                                                          const float* __restrict__ bn_shift, int relu,
                                                          float* __restrict__ y, int ldy, int cout) {
  const int col = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (col >= cout) return;
  const float acc = wave_dot(x + (size_t)blockIdx.y * ldx, w + (size_t)col * ldw + koff, k, lane);
  if (lane == 0) {
    float v = acc + (bias ? bias[col] : 0.0f);
    if (bn_scale) v = fmaf(v, bn_scale[col], bn_shift[col]);
    y[(size_t)blockIdx.y * ldy + col] = relu ? relu_nan(v) : v;
  }
}

// simple_setup.py:795-812: posterior = softmax(logits); with a prior: posterior * prior / train_prior,
// L1-normalised (:1001-1008); out_index = argmax (first maximum), out_max = its probability.  One workgroup.
__global__ __launch_bounds__(256) void orientation_posterior_kernel(const float* __restrict__ logits, int C,
                                                                    const float* __restrict__ prior,
                                                                    const float* __restrict__ train_prior,
                                                                    float* __restrict__ posterior,
                                                                    int* __restrict__ out_index,
                                                                    float* __restrict__ out_max) {
  __shared__ float red[256];
  __shared__ int red_i[256];
  const int tid = threadIdx.x;
  float m = -3.0e38f;
  for (int i = tid; i < C; i += 256) m = fmaxf(m, logits[i]);
  red[tid] = m;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) { if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]); __syncthreads(); }
  m = red[0];
  __syncthreads();
  float sum = 0.0f;
  for (int i = tid; i < C; i += 256) sum += expf(logits[i] - m);
  red[tid] = sum;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
  const float inv = 1.0f / red[0];
  __syncthreads();
  float l1 = 0.0f;
  for (int i = tid; i < C; i += 256) {
    float p = expf(logits[i] - m) * inv;
    if (prior) {
      p *= prior[i];
      if (train_prior) p /= train_prior[i];
      l1 += fabsf(p);
    }
    posterior[i] = p;
  }
  if (prior) {  // torch.nn.functional.normalize(p = 1): x / max(|x|_1, 1e-12)
    red[tid] = l1;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    const float k = 1.0f / fmaxf(red[0], 1e-12f);
    __syncthreads();
    for (int i = tid; i < C; i += 256) posterior[i] *= k;
  }
  __syncthreads();
  float best = -1.0f;
  int arg = 0x7fffffff;
  for (int i = tid; i < C; i += 256) {
    const float p = posterior[i];
    if (p > best) { best = p; arg = i; }
  }
  red[tid] = best; red_i[tid] = arg;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) {
      const float o = red[tid + s];
      const int oi = red_i[tid + s];
      if (o > red[tid] || (o == red[tid] && oi < red_i[tid])) { red[tid] = o; red_i[tid] = oi; }
    }
    __syncthreads();
  }
  if (tid == 0) { out_index[0] = red_i[0]; out_max[0] = red[0]; }
}

// The N largest entries of posterior[C], descending, equal values by ascending index, NaN as -inf (rank_key,
// common.hpp).  ONE workgroup, N rounds: round r takes the largest key below round r - 1's.  Keys of different cells
// differ, so "below the last one taken" leaves out exactly the cells already taken: nothing is marked, the posterior
// is only read, and a round is one strided pass (L2-resident: 144 KB at resolution 3), one wave reduction and one
// exchange of kTopkThreads / 64 keys through LDS.  Every thread ends a round with the same key, so the loop and its
// barriers are workgroup-uniform.
constexpr int kTopkThreads = 1024;
__global__ __launch_bounds__(kTopkThreads) void orientation_topk_kernel(const float* __restrict__ posterior, int C, int N,
                                                                        int* __restrict__ out_index,
                                                                        float* __restrict__ out_prob) {
  __shared__ unsigned long long wave_best[kTopkThreads / 64];
  const int tid = threadIdx.x;
  unsigned long long below = ~0ull;
  for (int r = 0; r < N; ++r) {
    unsigned long long best = 0;
    for (int i = tid; i < C; i += kTopkThreads) {
      const unsigned long long k = rank_key(posterior[i], i);
      if (k < below && k > best) best = k;
    }
    best = wave_max_u64(best);
    if ((tid & 63) == 0) wave_best[tid >> 6] = best;
    __syncthreads();
    best = wave_best[0];
#pragma unroll
    for (int w = 1; w < kTopkThreads / 64; ++w) best = wave_best[w] > best ? wave_best[w] : best;
    __syncthreads();   // (the next round's stores wait for these reads)
    if (best == 0) break;   // N > C: the host refuses it
    if (tid == 0) {
      const int i = (int)~(unsigned)best;
      out_index[r] = i;
      out_prob[r] = posterior[i];
    }
    below = best;
  }
}

// workgroup j: params[j] = params_one, with orientation = cam_quat (x) grid_quats[index[j]] (index clamped to the table)
__global__ __launch_bounds__(64) void init_hypotheses_kernel(const float* __restrict__ params_one, int n_params,
                                                             const float* __restrict__ grid_quats, int C,
                                                             const int* __restrict__ index,
                                                             const float* __restrict__ cam_quat,
                                                             float* __restrict__ params) {
  float* const row = params + (size_t)blockIdx.x * n_params;
  for (int i = threadIdx.x; i < n_params; i += 64)
    if (i < 3 || i > 6) row[i] = params_one[i];
  if (threadIdx.x != 0) return;
  const int i = min(max(index[blockIdx.x], 0), C - 1);
  const float q[4] = {grid_quats[4 * i], grid_quats[4 * i + 1], grid_quats[4 * i + 2], grid_quats[4 * i + 3]};
  const float c[4] = {cam_quat[0], cam_quat[1], cam_quat[2], cam_quat[3]};
  float qw[4];
  quat_mul_world(c, q, qw);
  for (int k = 0; k < 4; ++k) row[3 + k] = qw[k];
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

namespace {
int pointnet_layer_impl(const char* fn, const float* x, const int* row_count, int M, int cin, int ldx, const float* w,
                        int ldw, const float* cvec, const float* bn_scale, const float* bn_shift, const float* resid,
                        float* y, int ldy, int cout, float* colmax, int device, void* stream) {
  if (M < 1 || cin < 1 || cout < 1 || ldx < cin || ldw < cin || (y && ldy < cout))
    return fail(SDFR_E_INVALID, "%s: bad sizes M=%d cin=%d cout=%d", fn, M, cin, cout);
  if (!x || !w || !cvec || !bn_scale || !bn_shift || !colmax) return fail(SDFR_E_NULL, "%s: NULL pointer argument", fn);
  if (resid && !y) return fail(SDFR_E_NULL, "%s: a residual needs an output", fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  zero_words_async(colmax, (size_t)cout, st);
  // (a counted call does not know its rows: enough row blocks to fill the chip, striding over the real ones)
  const int row_blocks = (M + kPtsPerBlock - 1) / kPtsPerBlock;
  const int col_blocks = (cout + kColsPerBlock - 1) / kColsPerBlock;
  // (1024 workgroups: the point set of one mug view is ~330 row blocks, and workgroups that find no row cost the
  // dispatcher their launch all the same)
  const int gx = row_count ? std::min(row_blocks, std::max(1, 1024 / col_blocks)) : row_blocks;
  hipLaunchKernelGGL(pointnet_layer_kernel, dim3((unsigned)gx, (unsigned)col_blocks), dim3(256), 0, st, x, M, cin, ldx, w,
                     ldw, cvec, bn_scale, bn_shift, resid, y, ldy, cout, reinterpret_cast<int*>(colmax), row_count);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
}  // namespace

extern "C" int sdfr_pointnet_layer(const float* x, int M, int cin, int ldx, const float* w, int ldw,
                                   const float* cvec, const float* bn_scale, const float* bn_shift,
                                   const float* resid, float* y, int ldy, int cout, float* colmax, int device,
                                   void* stream) {
  return pointnet_layer_impl("sdfr_pointnet_layer", x, nullptr, M, cin, ldx, w, ldw, cvec, bn_scale, bn_shift, resid, y,
                             ldy, cout, colmax, device, stream);
}

extern "C" int sdfr_pointnet_layer_counted(const float* x, const int* row_count, int M_capacity, int cin, int ldx,
                                           const float* w, int ldw, const float* cvec, const float* bn_scale,
                                           const float* bn_shift, const float* resid, float* y, int ldy, int cout,
                                           float* colmax, int device, void* stream) {
  if (!row_count) return fail(SDFR_E_NULL, "sdfr_pointnet_layer_counted: row_count is NULL");
  return pointnet_layer_impl("sdfr_pointnet_layer_counted", x, row_count, M_capacity, cin, ldx, w, ldw, cvec, bn_scale,
                             bn_shift, resid, y, ldy, cout, colmax, device, stream);
}

extern "C" int sdfr_init_estimate(const float* head, int latent, const float* grid_quats, const int* index,
                                  const float* centroid, const float* cam_pos, const float* cam_quat, int mean_shape,
                                  int take_if_better, const float* posterior_max, float* best, float* params, int device,
                                  void* stream) {
  if (latent < 0 || latent > 1024) return fail(SDFR_E_INVALID, "sdfr_init_estimate: latent=%d", latent);
  if (!head || !cam_pos || !cam_quat || !params || (grid_quats && !index) || (take_if_better && (!posterior_max || !best)))
    return fail(SDFR_E_NULL, "sdfr_init_estimate: NULL pointer argument");
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(init_estimate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, head, latent, grid_quats, index,
                     centroid, cam_pos, cam_quat, mean_shape, take_if_better, posterior_max, best, params);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_linear_vec(const float* w, int ldw, int koff, const float* x, int k, const float* bias,
                               const float* bn_scale, const float* bn_shift, int relu, float* y, int cout,
                               int device, void* stream) {
  if (cout < 1 || k < 0 || koff < 0 || ldw < koff + k) return fail(SDFR_E_INVALID, "sdfr_linear_vec: bad sizes");
  if (!w || !y || (k > 0 && !x) || ((bn_scale == nullptr) != (bn_shift == nullptr)))
    return fail(SDFR_E_NULL, "sdfr_linear_vec: NULL pointer argument");
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(linear_rows_kernel, dim3((unsigned)((cout + 3) / 4), 1), dim3(256), 0, (hipStream_t)stream, w, ldw,
                     koff, x, k, k, bias, bn_scale, bn_shift, relu, y, cout, cout);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_linear_rows(const float* w, int ldw, int koff, const float* x, int ldx, int k, const float* bias,
                                const float* bn_scale, const float* bn_shift, int relu, float* y, int ldy, int cout,
                                int N, int device, void* stream) {
  if (N < 1 || N > 65535) return fail(SDFR_E_INVALID, "sdfr_linear_rows: N=%d rows (1 <= N <= 65535)", N);
  if (cout < 1 || k < 0 || koff < 0 || ldw < koff + k || ldx < k || ldy < cout)
    return fail(SDFR_E_INVALID, "sdfr_linear_rows: bad sizes cout=%d k=%d koff=%d ldw=%d ldx=%d ldy=%d", cout, k, koff,
                ldw, ldx, ldy);
  if (!w || !y || (k > 0 && !x) || ((bn_scale == nullptr) != (bn_shift == nullptr)))
    return fail(SDFR_E_NULL, "sdfr_linear_rows: NULL pointer argument");
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(linear_rows_kernel, dim3((unsigned)((cout + 3) / 4), (unsigned)N), dim3(256), 0,
                     (hipStream_t)stream, w, ldw, koff, x, ldx, k, bias, bn_scale, bn_shift, relu, y, ldy, cout);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_orientation_posterior(const float* logits, int C, const float* prior, const float* train_prior,
                                          float* posterior, int* out_index, float* out_max, int device,
                                          void* stream) {
  if (C < 1) return fail(SDFR_E_INVALID, "sdfr_orientation_posterior: C=%d", C);
  if (!logits || !posterior || !out_index || !out_max || (train_prior && !prior))
    return fail(SDFR_E_NULL, "sdfr_orientation_posterior: NULL pointer argument");
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(orientation_posterior_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, C, prior,
                     train_prior, posterior, out_index, out_max);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_orientation_topk(const float* posterior, int C, int N, int* out_index, float* out_prob, int device,
                                     void* stream) {
  if (N < 1 || N > SDFR_MAX_HYPOTHESES || C < N || C > (1 << 24))
    return fail(SDFR_E_INVALID, "sdfr_orientation_topk: N=%d of C=%d cells (1 <= N <= %d, N <= C <= 2^24)", N, C,
                SDFR_MAX_HYPOTHESES);
  if (!posterior || !out_index || !out_prob) return fail(SDFR_E_NULL, "sdfr_orientation_topk: NULL pointer argument");
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(orientation_topk_kernel, dim3(1), dim3(kTopkThreads), 0, (hipStream_t)stream, posterior, C, N,
                     out_index, out_prob);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_init_hypotheses(const float* params_one, int n_params, const float* grid_quats, int C,
                                    const int* index, int N, const float* cam_quat, float* params, int device,
                                    void* stream) {
  if (N < 1 || N > SDFR_MAX_HYPOTHESES || C < 1 || n_params < 8 || n_params > 8 + 1024)
    return fail(SDFR_E_INVALID, "sdfr_init_hypotheses: N=%d rows of n_params=%d from C=%d cells", N, n_params, C);
  if (!params_one || !grid_quats || !index || !cam_quat || !params)
    return fail(SDFR_E_NULL, "sdfr_init_hypotheses: NULL pointer argument");
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(init_hypotheses_kernel, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream, params_one, n_params,
                     grid_quats, C, index, cam_quat, params);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
