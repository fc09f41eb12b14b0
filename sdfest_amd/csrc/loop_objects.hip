// loop_objects.hip -- what the K-object loop (sdfr_loop_tail_objects, loop.hip) needs around its tail once an object
// has SEVERAL views and keeps the reference's inlier bookkeeping (include/sdfr.h, group 3):
//   sdfr_volumes_replicate     the K decoded SDF volumes, once per view: the render / sampler launches take one volume
//                              per view (sdf_view_stride), and view k V + v is object k from camera v
//   sdfr_volumes_sum_views     the K V gradient volumes those launches leave, summed per object for the batched VJP
//   sdfr_inlier_ratio_objects  sdfr_inlier_ratio (simple_setup.py:177-211) for K objects in two launches
// and, where the K rows are N hypotheses of one object, the way back to one answer:
//   sdfr_select_row            the row with the best score (one wave)
// The first three move bytes and do next to no arithmetic: a thread owns 4 consecutive floats of a row and moves them as one
// 16-byte access wherever the row starts on a 16-byte boundary (always for the loop's own buffers: R^3 and W H are
// multiples of 4 there), float by float where it does not (R odd: every row but each fourth starts off the boundary).
#include "common.hpp"

namespace sdfr {
namespace {

constexpr int kRowThreads = 256;
constexpr int kRowPasses = 4;                                    // 16-byte accesses per thread
constexpr size_t kRowChunk = (size_t)kRowThreads * kRowPasses * 4;   // floats of a row per workgroup

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// x[0..3] = row[i .. i + 3] (i a multiple of 4; elements at or past n are left alone)
__device__ __forceinline__ void load4(const float* __restrict__ row, bool vec, size_t i, size_t n, float (&x)[4]) {
  if (vec && i + 3 < n) {
    const float4 t = *reinterpret_cast<const float4*>(row + i);
    x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (i + j < n) x[j] = row[i + j];
}
__device__ __forceinline__ void store4(float* __restrict__ row, bool vec, size_t i, size_t n, const float (&x)[4]) {
  if (vec && i + 3 < n) {
    *reinterpret_cast<float4*>(row + i) = make_float4(x[0], x[1], x[2], x[3]);
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (i + j < n) row[i + j] = x[j];
}

// grid (chunks of a row, K): dst[k V + v] = src[k] for every v
__global__ __launch_bounds__(kRowThreads) void volumes_replicate_kernel(const float* __restrict__ src,
                                                                        float* __restrict__ dst, int V, size_t n) {
  const size_t k = blockIdx.y;
  const float* const s = src + k * n;
  const bool s_vec = aligned16(s);
#pragma unroll
  for (int pass = 0; pass < kRowPasses; ++pass) {
    const size_t i = (size_t)blockIdx.x * kRowChunk + ((size_t)pass * kRowThreads + threadIdx.x) * 4;
    if (i >= n) break;
    float x[4] = {0, 0, 0, 0};
    load4(s, s_vec, i, n, x);
    for (int v = 0; v < V; ++v) {
      float* const d = dst + (k * V + v) * n;
      store4(d, aligned16(d), i, n, x);
    }
  }
}

// grid (chunks of a row, K): dst[k] = ((src[k V] + src[k V + 1]) + ...), v ascending -- one fixed order of plain fp32
// additions per element, so the same bits on every run
__global__ __launch_bounds__(kRowThreads) void volumes_sum_views_kernel(const float* __restrict__ src,
                                                                        float* __restrict__ dst, int V, size_t n) {
  const size_t k = blockIdx.y;
  float* const d = dst + k * n;
  const bool d_vec = aligned16(d);
#pragma unroll
  for (int pass = 0; pass < kRowPasses; ++pass) {
    const size_t i = (size_t)blockIdx.x * kRowChunk + ((size_t)pass * kRowThreads + threadIdx.x) * 4;
    if (i >= n) break;
    const float* s = src + k * V * n;
    float acc[4] = {0, 0, 0, 0};
    load4(s, aligned16(s), i, n, acc);
    for (int v = 1; v < V; ++v) {
      s += n;
      float x[4] = {0, 0, 0, 0};
      load4(s, aligned16(s), i, n, x);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += x[j];
    }
    store4(d, d_vec, i, n, acc);
  }
}

// grid (chunks of 1024 pixels, K): counts[k][0] += #(|in - est| / in < thr), counts[k][1] += #(in != 0) -- the
// expression of inlier_count_kernel (loop.hip; the reference's, :182-186: a zero input gives inf or NaN, neither is
// below thr).  Integer counts: the order in which pixels and workgroups arrive does not matter.
constexpr int kInlierChunk = 1024;   // 256 threads x 4 consecutive pixels
__global__ __launch_bounds__(256) void inlier_count_objects_kernel(const float* __restrict__ depth_in,
                                                                   const float* __restrict__ depth_est,
                                                                   size_t est_stride, int npix, float rel_thr,
                                                                   int* __restrict__ counts) {
  const size_t k = blockIdx.y;
  const float* const in = depth_in + k * (size_t)npix;
  const float* const est = depth_est + k * est_stride;
  const size_t i = (size_t)blockIdx.x * kInlierChunk + (size_t)threadIdx.x * 4;
  float a[4] = {0, 0, 0, 0}, e[4] = {0, 0, 0, 0};
  int inl = 0, val = 0;
  if (i < (size_t)npix) {
    load4(in, aligned16(in), i, (size_t)npix, a);
    load4(est, aligned16(est), i, (size_t)npix, e);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i + j < (size_t)npix) {
        inl += (fabsf(a[j] - e[j]) / a[j] < rel_thr) ? 1 : 0;
        val += (a[j] != 0.0f) ? 1 : 0;
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    inl += __shfl_xor(inl, off, 64);
    val += __shfl_xor(val, off, 64);
  }
  // One atomic per workgroup: every workgroup of an object adds to the same two words, and atomics on one address
  // queue behind each other (one pair per wave, 2400 per 640x480 image, was what this kernel's time went to).  Both
  // counts in one 64-bit add where the pair is 8-byte aligned: neither half can carry (at most 2^31 - 1 pixels).
  __shared__ int wave_inl[4], wave_val[4];
  if ((threadIdx.x & 63) == 0) { wave_inl[threadIdx.x >> 6] = inl; wave_val[threadIdx.x >> 6] = val; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  inl = (wave_inl[0] + wave_inl[1]) + (wave_inl[2] + wave_inl[3]);
  val = (wave_val[0] + wave_val[1]) + (wave_val[2] + wave_val[3]);
  if (!inl && !val) return;
  int* const c = counts + 2 * k;
  if (((uintptr_t)c & 7) == 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(c),
              (unsigned long long)(unsigned)inl | ((unsigned long long)(unsigned)val << 32));
  } else {
    if (inl) atomicAdd(&c[0], inl);
    if (val) atomicAdd(&c[1], val);
  }
}

// workgroup k: inlier_update_kernel (loop.hip) on object k's counts, step counter, history row, state and parameters
__global__ __launch_bounds__(256) void inlier_update_objects_kernel(int* __restrict__ counts,
                                                                    const int* __restrict__ step,
                                                                    float* __restrict__ history, int max_history,
                                                                    float* __restrict__ state,
                                                                    const float* __restrict__ params, int n_params,
                                                                    float* __restrict__ best_params) {
  __shared__ int better;
  const size_t k = blockIdx.x;
  int* const c = counts + 2 * k;
  float* const s = state + 3 * k;
  if (threadIdx.x == 0) {
    const float ratio = (float)c[0] / (float)c[1];
    const int it = step[k];   // steps taken so far: Adam has run for this iteration already
    if (history && it >= 1 && it <= max_history) history[k * (size_t)max_history + it - 1] = ratio;
    better = (s[2] == 0.0f) || (ratio > s[0]);
    if (better) { s[0] = ratio; s[1] = (float)it; s[2] = 1.0f; }
    c[0] = 0; c[1] = 0;
  }
  __syncthreads();
  if (better && best_params)
    for (int i = threadIdx.x; i < n_params; i += blockDim.x)
      best_params[k * (size_t)n_params + i] = params[k * (size_t)n_params + i];
}

// ONE wave: lane j < N holds row j's score as a rank_key (common.hpp: the larger score, then the smaller j; NaN as
// -inf, so all-NaN gives row 0); after the wave maximum every lane knows the winner and the lanes copy its row
__global__ __launch_bounds__(64) void select_row_kernel(const float* __restrict__ score, int score_stride, int N,
                                                        const float* __restrict__ rows, int n,
                                                        float* __restrict__ out_row, int* __restrict__ out_index,
                                                        float* __restrict__ out_score) {
  const int lane = threadIdx.x;
  const unsigned long long key = wave_max_u64(lane < N ? rank_key(score[(size_t)lane * score_stride], lane) : 0ull);
  const int j = (int)~(unsigned)key;
  const float* const row = rows + (size_t)j * n;
  for (int i = lane; i < n; i += 64) out_row[i] = row[i];
  if (lane == 0) {
    out_index[0] = j;
    out_score[0] = score[(size_t)j * score_stride];
  }
}

// K rows of n floats as a (chunks, K) grid, or the reason why not
int rows_grid(const char* fn, int K, int V, size_t n, dim3* grid) {
  if (K < 0 || V < 1 || K > 65535 || (long long)K * V > 0x7fffffffLL)
    return fail(SDFR_E_INVALID, "%s: K=%d rows of V=%d views", fn, K, V);
  const size_t chunks = (n + kRowChunk - 1) / kRowChunk;
  if (chunks > 0x7fffffffULL) return fail(SDFR_E_INVALID, "%s: n=%zu floats per row exceed a launch", fn, n);
  *grid = dim3((unsigned)chunks, (unsigned)K);
  return 0;
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" int sdfr_volumes_replicate(const float* src, float* dst, int K, int V, size_t n, int device, void* stream) {
  dim3 grid;
  if (const int rc = rows_grid("sdfr_volumes_replicate", K, V, n, &grid)) return rc;
  if (K == 0 || n == 0) return 0;
  if (!src || !dst) return fail(SDFR_E_NULL, "sdfr_volumes_replicate: NULL pointer argument");
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(volumes_replicate_kernel, grid, dim3(kRowThreads), 0, (hipStream_t)stream, src, dst, V, n);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_volumes_sum_views(const float* src, float* dst, int K, int V, size_t n, int device, void* stream) {
  dim3 grid;
  if (const int rc = rows_grid("sdfr_volumes_sum_views", K, V, n, &grid)) return rc;
  if (K == 0 || n == 0) return 0;
  if (!src || !dst) return fail(SDFR_E_NULL, "sdfr_volumes_sum_views: NULL pointer argument");
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(volumes_sum_views_kernel, grid, dim3(kRowThreads), 0, (hipStream_t)stream, src, dst, V, n);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_inlier_ratio_objects(const float* depth_input, const float* depth_estimate, size_t estimate_stride,
                                         int K, int W, int H, float relative_threshold, const int* step, int* counts,
                                         float* history, int max_history, float* state, const float* params,
                                         int n_params, float* best_params, int device, void* stream) {
  const char* fn = "sdfr_inlier_ratio_objects";
  if (K < 0 || K > 65535 || W < 0 || H < 0 || (long long)W * H > 0x7fffffffLL || n_params < 0 || max_history < 0)
    return fail(SDFR_E_INVALID, "%s: bad sizes K=%d W=%d H=%d n_params=%d max_history=%d", fn, K, W, H, n_params,
                max_history);
  if (K > 1 && estimate_stride < (size_t)W * H)   // (one object: the stride is never used)
    return fail(SDFR_E_INVALID, "%s: estimate_stride=%zu is less than an image (%d x %d)", fn, estimate_stride, W, H);
  if (K == 0) return 0;
  if (!depth_input || !depth_estimate || !step || !counts || !state || (n_params > 0 && best_params && !params))
    return fail(SDFR_E_NULL, "%s: NULL pointer argument", fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int npix = W * H;
  if (npix > 0)
    hipLaunchKernelGGL(inlier_count_objects_kernel, dim3((npix + kInlierChunk - 1) / kInlierChunk, (unsigned)K),
                       dim3(256), 0, st, depth_input, depth_estimate, estimate_stride, npix, relative_threshold,
                       counts);
  hipLaunchKernelGGL(inlier_update_objects_kernel, dim3((unsigned)K), dim3(256), 0, st, counts, step, history,
                     max_history, state, params, n_params, best_params);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_select_row(const float* score, int score_stride, int N, const float* rows, int n, float* out_row,
                               int* out_index, float* out_score, int device, void* stream) {
  if (N < 1 || N > SDFR_MAX_HYPOTHESES || score_stride < 1 || n < 0)
    return fail(SDFR_E_INVALID, "sdfr_select_row: N=%d rows of n=%d, score_stride=%d (1 <= N <= %d)", N, n, score_stride,
                SDFR_MAX_HYPOTHESES);
  if (!score || !out_index || !out_score || (n > 0 && (!rows || !out_row)))
    return fail(SDFR_E_NULL, "sdfr_select_row: NULL pointer argument");
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(select_row_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, score, score_stride, N, rows, n,
                     out_row, out_index, out_score);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
