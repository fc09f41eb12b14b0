// initnet_eval.hip -- the initialisation network under eval() on N point sets at once, and the validation numbers of
// the reference's trainer (sdfest/initialization/scripts/train.py:344-374, :439-481):
//   sdfr_pointnet_layer_batch   the per-point layer with the set index in the grid: one launch per layer for the whole
//                               batch, ragged sets, a per-set cvec (a dense link's b + W[:, cin:] . max[n])
//   sdfr_pose_metrics           position / scale / geodesic / NLL sums of one batch into an fp64 record
// The layer is the tile of initnet_tile.hpp, the one the single-set kernel runs: row n of a batch has the bits of the
// single-set call on set n (the head and the per-set cvec are sdfr_linear_rows, initnet.hip).  Unlike the trainer's
// forward (initnet_train.hip) nothing is kept for a backward: no tape, running statistics folded into a scale and a
// shift, and the last layer leaves only its maxima.
#include "common.hpp"
#include "initnet_tile.hpp"

#include <climits>

namespace sdfr {
namespace {

// The per-point layer (pointnet_tile) for set blockIdx.z of x [N][M][ldx]: Y = relu((X W^T + c[n]) * s + t), optionally
// y = resid + Y, and colmax[n][col] = max over the set's rows of Y -- or of resid + Y (pool_resid: a residual link into
// the LAST layer, whose pooled values may be negative: order keys, decoded by pool_decode_kernel).
// grid (ceil(M / 64), ceil(cout / 64), N); a row tile lies inside one set; rows >= counts[n] are neither read into a
// result nor written.
template <bool pool_resid>
__global__ __launch_bounds__(256) void pointnet_layer_batch_kernel(
    const float* __restrict__ x, const int* __restrict__ counts, int M, int cin, int ldx, const float* __restrict__ w,
    int ldw, const float* __restrict__ cvec, int cvec_stride, const float* __restrict__ bn_scale,
    const float* __restrict__ bn_shift, const float* __restrict__ resid, float* __restrict__ y, int ldy, int cout,
    int* __restrict__ colmax) {
  __shared__ float xs[kPtsPerBlock * kTileLd];
  __shared__ float ws[kColsPerBlock * kTileLd];
  __shared__ int wave_max[4][kColsPerBlock];
  f32x4 acc[4];                                 // (pointnet_tile's accumulator: own_acc)
  const int n = blockIdx.z;
  const int rows = counts ? min(max(counts[n], 0), M) : M;
  const int p0 = blockIdx.x * kPtsPerBlock;
  if (p0 >= rows) return;                       // (workgroup-uniform, in front of every barrier)
  x += (size_t)n * M * ldx;
  if (y) y += (size_t)n * M * ldy;
  if (resid) resid += (size_t)n * M * ldy;
  cvec += (size_t)n * cvec_stride;
  colmax += (size_t)n * cout;
  pointnet_tile<pool_resid, false>(xs, ws, wave_max, &acc, x, rows, p0, cin, ldx, w, ldw, cvec, bn_scale, bn_shift, resid,
                                   y, ldy, cout, colmax);
}

static __global__ void fill_int_kernel(int* __restrict__ p, size_t n, int value) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = value;
}

// order keys -> floats; a set without rows: 0
static __global__ void pool_decode_kernel(int* __restrict__ p, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int k = p[i];
  p[i] = k == INT_MIN ? 0 : (k >= 0 ? k : k ^ 0x7fffffff);
}

// One wave per sample: sample[n] = {|p - p*|, |s - s*|, 2 acos(clip(|q . q*|, 0, 1)), logsumexp(logits) - logits[target]}
// in fp64 from the fp32 row.  q = grid_quats[first maximum of the logits] (orientation_posterior_kernel's rule) or the
// row's quaternion normalised.
__global__ __launch_bounds__(256) void pose_metrics_sample_kernel(
    const float* __restrict__ out, int N, int ld, int L, int n_cells, const float* __restrict__ grid_quats,
    const float* __restrict__ position, const float* __restrict__ scale, const float* __restrict__ quat,
    const int* __restrict__ index, double* __restrict__ sample) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  const float* o = out + (size_t)n * ld;
  double q[4], nll = 0.0;
  if (n_cells > 0) {
    const float* lg = o + L + 4;
    float best = -INFINITY;
    int arg = INT_MAX;
    for (int i = lane; i < n_cells; i += 64)
      if (lg[i] > best) { best = lg[i]; arg = i; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float ob = __shfl_xor(best, off, 64);
      const int oa = __shfl_xor(arg, off, 64);
      if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (arg < 0 || arg >= n_cells) arg = 0;          // (logits that are all NaN: a cell inside the table)
    for (int k = 0; k < 4; ++k) q[k] = grid_quats[4 * (size_t)arg + k];
    if (index) {
      double sum = 0.0;
      for (int i = lane; i < n_cells; i += 64) sum += exp((double)lg[i] - (double)best);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
      const int target = min(max(index[n], 0), n_cells - 1);
      nll = (double)best + log(sum) - (double)lg[target];
    }
  } else {   // sdf_pose_network.py:97-101
    double s = 0.0;
    for (int k = 0; k < 4; ++k) { q[k] = o[L + 4 + k]; s += q[k] * q[k]; }
    s = sqrt(s);
    for (int k = 0; k < 4; ++k) q[k] /= s;
  }
  if (lane != 0) return;
  double d2 = 0.0, dq = 0.0;
  for (int k = 0; k < 3; ++k) { const double d = (double)o[L + k] - (double)position[3 * (size_t)n + k]; d2 += d * d; }
  for (int k = 0; k < 4; ++k) dq += q[k] * (double)quat[4 * (size_t)n + k];
  dq = fabs(dq);
  if (dq > 1.0) dq = 1.0;                            // torch.clip: a NaN stays one
  double* rec = sample + 4 * (size_t)n;
  rec[0] = sqrt(d2);
  rec[1] = fabs((double)o[L + 3] - (double)scale[n]);
  rec[2] = 2.0 * acos(dq);
  rec[3] = nll;
}

// one thread: the N sample records onto the caller's record, in sample order
__global__ void pose_metrics_sum_kernel(const double* __restrict__ sample, int N, double* __restrict__ record) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double acc[4] = {record[0], record[1], record[2], record[3]};
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < 4; ++k) acc[k] += sample[4 * (size_t)n + k];
  for (int k = 0; k < 4; ++k) record[k] = acc[k];
  record[4] += (double)N;
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" int sdfr_pointnet_layer_batch(const float* x, const int* counts, int N, int M_capacity, int cin, int ldx,
                                         const float* w, int ldw, const float* cvec, int cvec_stride,
                                         const float* bn_scale, const float* bn_shift, const float* resid, float* y,
                                         int ldy, int cout, int pool_resid, float* colmax, int device, void* stream) {
  const char* fn = "sdfr_pointnet_layer_batch";
  if (N < 1 || N > 65535 || M_capacity < 1 || (long long)N * M_capacity > (1ll << 30))
    return fail(SDFR_E_INVALID, "%s: N=%d sets of M_capacity=%d rows (1 <= N <= 65535, N M <= 2^30)", fn, N, M_capacity);
  if (cin < 1 || cout < 1 || ldx < cin || ldw < cin || ((y || resid) && ldy < cout))
    return fail(SDFR_E_INVALID, "%s: bad sizes cin=%d cout=%d ldx=%d ldw=%d ldy=%d", fn, cin, cout, ldx, ldw, ldy);
  if (cvec_stride != 0 && cvec_stride != cout)
    return fail(SDFR_E_INVALID, "%s: cvec_stride=%d is neither 0 (shared) nor cout (per set)", fn, cvec_stride);
  if (!x || !w || !cvec || !bn_scale || !bn_shift || !colmax) return fail(SDFR_E_NULL, "%s: NULL pointer argument", fn);
  if (pool_resid ? !resid : (resid && !y))
    return fail(SDFR_E_NULL, pool_resid ? "%s: pool_resid needs a residual" : "%s: a residual needs an output", fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const size_t words = (size_t)N * cout;
  int* cm = reinterpret_cast<int*>(colmax);
  hipLaunchKernelGGL(fill_int_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, cm, words,
                     pool_resid ? INT_MIN : 0);
  const unsigned row_blocks = (unsigned)((M_capacity + kPtsPerBlock - 1) / kPtsPerBlock);
  const unsigned col_blocks = (unsigned)((cout + kColsPerBlock - 1) / kColsPerBlock);
  hipLaunchKernelGGL(pool_resid ? pointnet_layer_batch_kernel<true> : pointnet_layer_batch_kernel<false>,
                     dim3(row_blocks, col_blocks, (unsigned)N), dim3(256), 0, st, x, counts, M_capacity, cin, ldx, w, ldw,
                     cvec, cvec_stride, bn_scale, bn_shift, resid, y, ldy, cout, cm);
  if (pool_resid)
    hipLaunchKernelGGL(pool_decode_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, cm, words);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" size_t sdfr_pose_metrics_workspace_bytes(int N) { return N < 1 ? 0 : (size_t)N * 4 * sizeof(double); }

extern "C" int sdfr_pose_metrics(const float* out, int N, int ld_out, int latent, int n_cells, const float* grid_quats,
                                 const float* position, const float* scale, const float* quat,
                                 const int* orientation_index, double* record, void* workspace, size_t workspace_bytes,
                                 int device, void* stream) {
  const char* fn = "sdfr_pose_metrics";
  if (N < 1 || latent < 0 || n_cells < 0) return fail(SDFR_E_INVALID, "%s: N=%d latent=%d n_cells=%d", fn, N, latent, n_cells);
  if (ld_out < latent + 4 + (n_cells ? n_cells : 4))
    return fail(SDFR_E_INVALID, "%s: ld_out=%d is shorter than an output row (%d)", fn, ld_out,
                latent + 4 + (n_cells ? n_cells : 4));
  if (!out || !position || !scale || !quat || !record || !workspace) return fail(SDFR_E_NULL, "%s: NULL pointer argument", fn);
  if (n_cells > 0 && !grid_quats) return fail(SDFR_E_NULL, "%s: n_cells=%d needs grid_quats", fn, n_cells);
  if (((uintptr_t)workspace | (uintptr_t)record) & 7) return fail(SDFR_E_INVALID, "%s: record and workspace must be 8-byte aligned", fn);
  if (workspace_bytes < sdfr_pose_metrics_workspace_bytes(N))
    return fail(SDFR_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes,
                sdfr_pose_metrics_workspace_bytes(N));
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  double* sample = static_cast<double*>(workspace);
  hipLaunchKernelGGL(pose_metrics_sample_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, out, N, ld_out, latent,
                     n_cells, grid_quats, position, scale, quat, n_cells > 0 ? orientation_index : nullptr, sample);
  hipLaunchKernelGGL(pose_metrics_sum_kernel, dim3(1), dim3(64), 0, st, sample, N, record);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
