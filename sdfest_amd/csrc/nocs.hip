// nocs.hip -- pose and scale of NOCS-annotated objects (include/sdfr.h, group 12): the reference's
// initialization/datasets/nocs_dataset.py::_estimate_object and nocs_utils.estimate_similarity_transform, for K objects
// per call, ragged through device offsets [K + 1].
//
// Correspondences (sdfr_nocs_count, sdfr_nocs_correspondences), the two passes of the depth kernels (loop.hip):
//   1. nocs_count_kernel(nblk, K)        -- valid pixels and the largest valid depth per block of 1024 pixels
//   2. nocs_count_reduce_kernel(K)       -- one wave per object: counts[k], max_depth[k]
//   3. nocs_compact_kernel(nblk, K)      -- row-major compaction: source = NOCS colour, target = back-projection
//
// Fit (sdfr_similarity_ransac), all arithmetic fp64:
//   1. ransac_hypotheses_kernel(K)       -- mean norms -> pass_t, stop_t; lane i < 100: Umeyama of sample i's 5 pairs
//   2. ransac_evaluate_kernel(chunks, K) -- LANES ARE HYPOTHESES: a workgroup of two waves stages kEvalPts points
//                                           in LDS as fp64 and every lane runs its own transform (24 VGPRs) over them
//                                           in point order; every lane reads the same LDS address (a broadcast), no
//                                           lane ever needs another's sum.  One partial sum per (chunk, hypothesis).
//   3. ransac_finish_kernel(K)           -- residual_i = sqrt(sum of the chunk partials, in chunk order); the
//                                           reference's sequential loop replayed by one lane; inliers of the winner;
//                                           Umeyama over the inliers (two passes: centroids, then covariance)
// Every sum has an order that depends on the object's point count alone: a chunk is kEvalPts consecutive points
// of the OBJECT, partials are added in chunk order, the block reductions add lane-strided sums in lane order.  A batch
// therefore equals its single calls bit for bit, wherever an object stands in it.
//
// Why lanes are hypotheses and not points: with points on the lanes every hypothesis ends in a 64-lane fp64 reduction
// (100 of them per wave, 12 DPP/permute steps each) or each lane keeps 100 accumulators (200 VGPRs); with hypotheses on
// the lanes the inner loop is three 16-byte LDS broadcasts and 15 fp64 operations per point and nothing else.  100 of
// 128 lanes work.
//
// Sample indices (sdfr_nocs_sample_indices): Philox-4x32-10, key = the object's seed, counter = {iteration, draw,
// attempt, kNocsStream}; index = floor(word * N / 2^32); a draw that repeats an earlier one of its row is drawn again
// with the next attempt (after kNocsMaxAttempts: the smallest unused index, so the loop is bounded).
#include "common.hpp"
#include "philox.hpp"

namespace sdfr {
namespace {

constexpr int kHyp = SDFR_NOCS_HYPOTHESES;   // RANSAC iterations (nocs_utils.py:57)
constexpr int kHypPad = 128;                 // lanes of the evaluation workgroup = stride of the per-hypothesis tables
// Points a workgroup of the evaluation stages in LDS as fp64 (48 bytes each) and walks.  NOT a build-time tunable: it is
// the unit of the residual's summation order, so another value gives other last bits.  128: a NOCS object of ~4 000
// points gives ~32 workgroups, a frame's five objects ~160 for 256 CUs (not timed against other values).
constexpr int kEvalPts = 128;
constexpr int kBlock = 256;
constexpr int kCountPix = 1024;              // pixels per workgroup of the correspondence passes (4 per lane)
constexpr unsigned kNocsStream = 0x4E4F4353u;   // counter word 3 ("NOCS"), apart from the other Philox streams
constexpr int kNocsMaxAttempts = 64;
static_assert(kHyp <= kHypPad && kHypPad == 128, "two waves hold the hypotheses");

// ---- correspondences ---------------------------------------------------------------------------------------------
// the reference's `(mask == id) * depth != 0` (nocs_dataset.py:680-683): a product, so a NaN or infinite depth is
// "valid" wherever it stands
__device__ __forceinline__ bool nocs_valid(unsigned char m, int id, float z) {
  return ((m == id) ? 1.0f : 0.0f) * z != 0.0f;
}

// grid (nblk, K)
__global__ __launch_bounds__(kBlock) void nocs_count_kernel(const float* __restrict__ depth,
                                                            const unsigned char* __restrict__ mask, int npix,
                                                            const int* __restrict__ ids, int nblk,
                                                            int* __restrict__ block_count,
                                                            float* __restrict__ block_max) {
  __shared__ int cs[4];
  __shared__ float ms[4];
  const int k = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int id = ids[k];
  const int p0 = blk * kCountPix + tid * 4;
  int c = 0;
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = p0 + j;
    if (p < npix && nocs_valid(mask[p], id, depth[p])) {
      ++c;
      mx = fmaxf(mx, depth[p]);   // (fmaxf skips a NaN depth, torch.max would return it; depth images are decoded integers)
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    c += __shfl_xor(c, off, 64);
    mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  }
  if (lane == 0) { cs[wave] = c; ms[wave] = mx; }
  __syncthreads();
  if (tid == 0) {
    block_count[(size_t)k * nblk + blk] = cs[0] + cs[1] + cs[2] + cs[3];
    block_max[(size_t)k * nblk + blk] = fmaxf(fmaxf(ms[0], ms[1]), fmaxf(ms[2], ms[3]));
  }
}

// grid K, one wave
__global__ __launch_bounds__(64) void nocs_count_reduce_kernel(const int* __restrict__ block_count,
                                                               const float* __restrict__ block_max, int nblk,
                                                               int* __restrict__ counts,
                                                               float* __restrict__ max_depth) {
  const int k = blockIdx.x, lane = threadIdx.x;
  int c = 0;
  float mx = -INFINITY;
  for (int i = lane; i < nblk; i += 64) {
    c += block_count[(size_t)k * nblk + i];
    mx = fmaxf(mx, block_max[(size_t)k * nblk + i]);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    c += __shfl_xor(c, off, 64);
    mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  }
  if (lane == 0) {
    counts[k] = c;
    max_depth[k] = c > 0 ? mx : 0.0f;
  }
}

// grid (nblk, K): the valid pixels of object k in row-major order, written at offsets[k] + rank
__global__ __launch_bounds__(kBlock) void nocs_compact_kernel(
    const float* __restrict__ depth, const unsigned char* __restrict__ mask, const unsigned char* __restrict__ nocs,
    int channels, int W, int npix, const int* __restrict__ ids, int nblk, const int* __restrict__ block_count,
    const long long* __restrict__ offsets, long long capacity, float rfx, float rfy, float cx0, float cy0,
    float* __restrict__ source, float* __restrict__ target) {
  __shared__ int wsum[4];
  __shared__ int base_s;
  const int k = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* bc = block_count + (size_t)k * nblk;
  if (bc[blk] == 0) return;   // workgroup-uniform
  if (wave == 0) {
    int s = 0;
    for (int i = lane; i < blk; i += 64) s += bc[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) base_s = s;
  }
  const int id = ids[k];
  const int p0 = blk * kCountPix + tid * 4;
  float z[4];
  bool ok[4];
  int c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = p0 + j;
    z[j] = p < npix ? depth[p] : 0.0f;
    ok[j] = p < npix && nocs_valid(mask[p], id, z[j]);
    c += ok[j] ? 1 : 0;
  }
  int incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int before = incl - c;
  for (int w = 0; w < wave; ++w) before += wsum[w];
  // the caller's offsets are clamped to its buffers: a row beyond `capacity` is never written
  const long long begin = offsets[k], end = offsets[k + 1];
  long long at = begin + base_s + before;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // every operation rounds on its own, as the reference's separate torch / numpy operations do
#pragma clang fp contract(off)
    if (!ok[j]) continue;
    if (at >= 0 && at < end && at < capacity) {
      const int p = p0 + j;
      const int row = p / W, col = p - row * W;
      const unsigned char* c3 = nocs + (size_t)p * channels;
      float* s = source + 3 * at;
      float* t = target + 3 * at;
      s[0] = (float)c3[0] / 255.0f - 0.5f;
      s[1] = (float)c3[1] / 255.0f - 0.5f;
      s[2] = (1.0f - (float)c3[2] / 255.0f) - 0.5f;   // the z flip of _load_nocs_map (:670)
      t[0] = (((float)col - cx0) * z[j]) * rfx;        // depth_compact_kernel's expressions, OpenCV signs
      t[1] = (((float)row - cy0) * z[j]) * rfy;
      t[2] = z[j];
    }
    ++at;
  }
}

// ---- fp64 3 x 3 algebra ------------------------------------------------------------------------------------------
struct D3 {
  double x, y, z;
};
__device__ __forceinline__ D3 d3(double x, double y, double z) { return D3{x, y, z}; }
__device__ __forceinline__ double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 dcross(D3 a, D3 b) {
  return d3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ D3 dunit(D3 a, D3 fallback) {
  const double n = sqrt(ddot(a, a));
  return n > 0.0 ? d3(a.x / n, a.y / n, a.z / n) : fallback;
}

template <typename T>
__device__ __forceinline__ D3 load_point(const T* __restrict__ p, long long i) {
  return d3((double)p[3 * i], (double)p[3 * i + 1], (double)p[3 * i + 2]);
}

// one rotation of the one-sided (Hestenes) Jacobi SVD on the columns a, b of W = A V and of V
__device__ __forceinline__ bool jacobi_pair(D3& a, D3& b, D3& va, D3& vb) {
  const double alpha = ddot(a, a), beta = ddot(b, b), gamma = ddot(a, b);
  if (!(fabs(gamma) > 1e-17 * sqrt(alpha * beta))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  const D3 a2 = d3(c * a.x - s * b.x, c * a.y - s * b.y, c * a.z - s * b.z);
  const D3 b2 = d3(s * a.x + c * b.x, s * a.y + c * b.y, s * a.z + c * b.z);
  const D3 va2 = d3(c * va.x - s * vb.x, c * va.y - s * vb.y, c * va.z - s * vb.z);
  const D3 vb2 = d3(s * va.x + c * vb.x, s * va.y + c * vb.y, s * va.z + c * vb.z);
  a = a2; b = b2; va = va2; vb = vb2;
  return true;
}

// status of a fit (also the per-hypothesis flags)
constexpr int kFitOk = 0, kFitZeroVariance = 1, kFitNan = 2;

// The tail of _estimate_similarity_umeyama (nocs_utils.py:209-241) from the centroids, the covariance (row-major,
// cov[i][j] = mean(ct_i * cs_j)) and var_p = sum of the source's population variances.  T = the 3 x 4 transform
// [scale * R | t], row-major; rot / scale: nullable.  With the Jacobi columns sorted, R is formed as
//     u1 v1^T + u2 v2^T + u3 v3^T,   u3 = det(V) * (u1 x u2),   v3 = the third column of V,
// and the scale takes sigma3 with the sign of u3 . (A v3).  Contract: whenever the fit is kFitOk, R is a ROTATION
// (orthogonal, det R = det(V)^2 = +1 by construction), whatever the covariance's rank.  For a covariance of full rank
// this is the reference's U S V^T, S = diag(1, 1, sign det(cov)): u1 x u2 is +-(A v3) / sigma3, and the sign of
// u3 . (A v3) is that of det(cov).  For a covariance of rank two or one (an exactly planar or collinear source set,
// e.g. one flat face of 8-bit NOCS colours) a rotation and its mirror image fit equally well and det(cov) is zero but
// for rounding; the reference then returns either by LAPACK's rounding, this returns the rotation.
__device__ int umeyama_finish(D3 cs, D3 ct, const double* cov, double var_p, double* T, double* rot, double* scale) {
  bool nan = false;
#pragma unroll
  for (int i = 0; i < 9; ++i) nan = nan || (cov[i] != cov[i]);
  if (nan) return kFitNan;              // "There are NANs in the input." (:211-215)
  // columns of A = cov
  D3 w0 = d3(cov[0], cov[3], cov[6]), w1 = d3(cov[1], cov[4], cov[7]), w2 = d3(cov[2], cov[5], cov[8]);
  D3 v0 = d3(1, 0, 0), v1 = d3(0, 1, 0), v2 = d3(0, 0, 1);
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool any = jacobi_pair(w0, w1, v0, v1);
    any = jacobi_pair(w0, w2, v0, v2) || any;
    any = jacobi_pair(w1, w2, v1, v2) || any;
    if (!any) break;
  }
  double s0 = sqrt(ddot(w0, w0)), s1 = sqrt(ddot(w1, w1)), s2 = sqrt(ddot(w2, w2));
  // descending order
  D3 tw, tv;
  double ts;
#define SDFR_SWAP(i, j)                                                        \
  if (s##i < s##j) {                                                           \
    tw = w##i; w##i = w##j; w##j = tw; tv = v##i; v##i = v##j; v##j = tv;      \
    ts = s##i; s##i = s##j; s##j = ts;                                         \
  }
  SDFR_SWAP(0, 1) SDFR_SWAP(0, 2) SDFR_SWAP(1, 2)
#undef SDFR_SWAP
  const D3 u0 = dunit(w0, d3(1, 0, 0));
  D3 u1 = dunit(w1, d3(0, 1, 0));
  // (re-orthogonalised against u0: exact for converged columns, and a rank-one covariance still gets a frame)
  const double p01 = ddot(u0, u1);
  u1 = dunit(d3(u1.x - p01 * u0.x, u1.y - p01 * u0.y, u1.z - p01 * u0.z), dunit(dcross(u0, d3(0, 0, 1)), d3(0, 1, 0)));
  // V is a product of plane rotations and the column swaps above: det(V) = +-1, read off its triple product
  D3 u2 = dcross(u0, u1);
  if (ddot(v0, dcross(v1, v2)) < 0.0) u2 = d3(-u2.x, -u2.y, -u2.z);
  const double sign = ddot(u2, w2) < 0.0 ? -1.0 : 1.0;
  if (var_p == 0.0) return kFitZeroVariance;   // PoseEstimationError (:226-229)
  const double sc = 1.0 / var_p * (s0 + s1 + sign * s2);
  const D3 u[3] = {u0, u1, u2};
  const D3 v[3] = {v0, v1, v2};
  double R[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double vc0 = c == 0 ? v[0].x : c == 1 ? v[0].y : v[0].z;
    const double vc1 = c == 0 ? v[1].x : c == 1 ? v[1].y : v[1].z;
    const double vc2 = c == 0 ? v[2].x : c == 1 ? v[2].y : v[2].z;
    R[0 + c] = u[0].x * vc0 + u[1].x * vc1 + u[2].x * vc2;
    R[3 + c] = u[0].y * vc0 + u[1].y * vc1 + u[2].y * vc2;
    R[6 + c] = u[0].z * vc0 + u[1].z * vc1 + u[2].z * vc2;
  }
  const double c3[3] = {cs.x, cs.y, cs.z}, t3[3] = {ct.x, ct.y, ct.z};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double a = sc * R[3 * r], b = sc * R[3 * r + 1], c = sc * R[3 * r + 2];
    T[4 * r] = a; T[4 * r + 1] = b; T[4 * r + 2] = c;
    T[4 * r + 3] = t3[r] - (a * c3[0] + b * c3[1] + c * c3[2]);
  }
  if (rot) {
#pragma unroll
    for (int i = 0; i < 9; ++i) rot[i] = R[i];
  }
  if (scale) *scale = sc;
  return kFitOk;
}

struct Range {
  long long begin;
  int n;
  bool truncated;   // the object has more than max_n rows: the fit answers SDFR_NOCS_TRUNCATED
};
// the caller's offsets, clamped to its buffers (no offset makes a kernel read outside [0, total))
__device__ __forceinline__ Range object_range(const long long* __restrict__ offsets, int k, long long total, int max_n) {
  long long b = offsets[k], e = offsets[k + 1];
  b = b < 0 ? 0 : (b > total ? total : b);
  e = e < b ? b : (e > total ? total : e);
  const long long n = e - b;
  return Range{b, (int)(n > max_n ? max_n : n), n > max_n};
}

// sum over the workgroup's kBlock lanes of M values per lane, lane order: red [M][kBlock] in LDS; the result is in
// red[m * kBlock] for every lane after the call
template <int M>
__device__ __forceinline__ void block_sum(double (*red)[kBlock], const double* mine) {
  const int tid = threadIdx.x;
  __syncthreads();   // the previous use of `red` is over
#pragma unroll
  for (int m = 0; m < M; ++m) red[m][tid] = mine[m];
  __syncthreads();
  if (tid < M) {
    double s = 0.0;
    for (int i = 0; i < kBlock; ++i) s += red[tid][i];
    red[tid][0] = s;
  }
  __syncthreads();
}

// per-object header of the workspace
struct FitHeader {
  double pass_t, stop_t;
};

// grid K
template <typename T>
__global__ __launch_bounds__(kBlock) void ransac_hypotheses_kernel(const T* __restrict__ source,
                                                                   const T* __restrict__ target,
                                                                   const long long* __restrict__ offsets,
                                                                   long long total, int max_n,
                                                                   const int* __restrict__ samples,
                                                                   FitHeader* __restrict__ header,
                                                                   double* __restrict__ transforms,
                                                                   int* __restrict__ flags) {
  __shared__ double red[2][kBlock];
  const int k = blockIdx.x, tid = threadIdx.x;
  const Range r = object_range(offsets, k, total, max_n);
  const T* src = source + 3 * r.begin;
  const T* tgt = target + 3 * r.begin;
  // thresholds (nocs_utils.py:50-56) from the mean norms
  double mine[2] = {0.0, 0.0};
  for (int i = tid; i < r.n; i += kBlock) {
    const D3 s = load_point(src, i), t = load_point(tgt, i);
    mine[0] += sqrt(ddot(s, s));
    mine[1] += sqrt(ddot(t, t));
  }
  block_sum<2>(red, mine);
  if (tid == 0) {
    const double sn = red[0][0] / (double)r.n, tn = red[1][0] / (double)r.n;
    const double ts = tn / sn, st = sn / tn;
    const double pass_t = (st > ts ? st : ts) * 0.01;
    header[k].pass_t = pass_t;
    header[k].stop_t = pass_t / 100;
  }
  if (tid >= kHyp) return;
  double* T12 = transforms + ((size_t)k * kHypPad + tid) * 12;
  int flag = kFitNan;
  if (r.n >= 5) {
    D3 s[5], t[5];
    D3 cs = d3(0, 0, 0), ct = d3(0, 0, 0);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      int idx = samples[((size_t)k * kHyp + tid) * 5 + j];
      idx = idx < 0 ? 0 : (idx >= r.n ? r.n - 1 : idx);
      s[j] = load_point(src, idx);
      t[j] = load_point(tgt, idx);
      cs = d3(cs.x + s[j].x, cs.y + s[j].y, cs.z + s[j].z);
      ct = d3(ct.x + t[j].x, ct.y + t[j].y, ct.z + t[j].z);
    }
    cs = d3(cs.x / 5, cs.y / 5, cs.z / 5);
    ct = d3(ct.x / 5, ct.y / 5, ct.z / 5);
    double cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double var = 0.0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const D3 a = d3(t[j].x - ct.x, t[j].y - ct.y, t[j].z - ct.z);
      const D3 b = d3(s[j].x - cs.x, s[j].y - cs.y, s[j].z - cs.z);
      cov[0] += a.x * b.x; cov[1] += a.x * b.y; cov[2] += a.x * b.z;
      cov[3] += a.y * b.x; cov[4] += a.y * b.y; cov[5] += a.y * b.z;
      cov[6] += a.z * b.x; cov[7] += a.z * b.y; cov[8] += a.z * b.z;
      var += ddot(b, b);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) cov[i] /= 5;
    var /= 5;
    double Tl[12];
    flag = umeyama_finish(cs, ct, cov, var, Tl, nullptr, nullptr);
    if (flag == kFitOk) {
#pragma unroll
      for (int i = 0; i < 12; ++i) T12[i] = Tl[i];
    }
  }
  if (flag != kFitOk) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int i = 0; i < 12; ++i) T12[i] = qnan;
  }
  flags[(size_t)k * kHypPad + tid] = flag;
}

// grid (chunks, K), kHypPad lanes: partial[k][chunk][lane] = sum over the chunk's points of |target - T_lane source|^2
template <typename T>
__global__ __launch_bounds__(kHypPad) void ransac_evaluate_kernel(const T* __restrict__ source,
                                                                  const T* __restrict__ target,
                                                                  const long long* __restrict__ offsets,
                                                                  long long total, int max_n, int chunks,
                                                                  const double* __restrict__ transforms,
                                                                  double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) double pts[kEvalPts][6];
  const int k = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const Range r = object_range(offsets, k, total, max_n);
  const int first = chunk * kEvalPts;
  if (first >= r.n) return;   // workgroup-uniform
  const int cnt = r.n - first < kEvalPts ? r.n - first : kEvalPts;
  for (int i = tid; i < cnt; i += kHypPad) {
    const D3 s = load_point(source + 3 * r.begin, first + i), t = load_point(target + 3 * r.begin, first + i);
    pts[i][0] = s.x; pts[i][1] = s.y; pts[i][2] = s.z;
    pts[i][3] = t.x; pts[i][4] = t.y; pts[i][5] = t.z;
  }
  double M[12];
  const double* T12 = transforms + ((size_t)k * kHypPad + (tid < kHyp ? tid : 0)) * 12;
#pragma unroll
  for (int i = 0; i < 12; ++i) M[i] = T12[i];
  __syncthreads();
  double acc = 0.0;
  for (int i = 0; i < cnt; ++i) {
    const double sx = pts[i][0], sy = pts[i][1], sz = pts[i][2];
    const double dx = pts[i][3] - (M[0] * sx + M[1] * sy + M[2] * sz + M[3]);
    const double dy = pts[i][4] - (M[4] * sx + M[5] * sy + M[6] * sz + M[7]);
    const double dz = pts[i][5] - (M[8] * sx + M[9] * sy + M[10] * sz + M[11]);
    acc += dx * dx + dy * dy + dz * dz;
  }
  partial[((size_t)k * chunks + chunk) * kHypPad + tid] = acc;
}

// grid K
template <typename T>
__global__ __launch_bounds__(kBlock) void ransac_finish_kernel(
    const T* __restrict__ source, const T* __restrict__ target, const long long* __restrict__ offsets, long long total,
    int max_n, int chunks, const FitHeader* __restrict__ header, const double* __restrict__ transforms,
    const int* __restrict__ flags, const double* __restrict__ partial, unsigned char* __restrict__ inlier,
    double* __restrict__ position, double* __restrict__ rotation, double* __restrict__ scale,
    double* __restrict__ transform, double* __restrict__ inlier_ratio, int* __restrict__ best_iteration,
    int* __restrict__ iterations_run, int* __restrict__ status, unsigned char* __restrict__ inlier_mask) {
  __shared__ double red[12][kBlock];
  __shared__ double residual[kHypPad];
  __shared__ int sel[3];   // winner, iterations run, status so far
  const int k = blockIdx.x, tid = threadIdx.x;
  const Range r = object_range(offsets, k, total, max_n);
  const T* src = source + 3 * r.begin;
  const T* tgt = target + 3 * r.begin;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  if (tid < kHyp) {
    const int my_chunks = (r.n + kEvalPts - 1) / kEvalPts;
    double s = 0.0;
    for (int c = 0; c < my_chunks; ++c) s += partial[((size_t)k * chunks + c) * kHypPad + tid];
    residual[tid] = sqrt(s);
  }
  __syncthreads();
  if (tid == 0) {
    // _get_ransac_inliers (nocs_utils.py:111-131), iteration by iteration
    int winner = -1, ran = 0, st = SDFR_NOCS_OK;
    if (r.truncated) {
      st = SDFR_NOCS_TRUNCATED;   // max_n is too small for this object: no result, not one of a part of its rows
    } else if (r.n < 5) {
      st = SDFR_NOCS_NONE;   // "Not enough point correspondences" (:41-43)
    } else {
      double best = 1e10;
      const double stop_t = header[k].stop_t;
      for (int i = 0; i < kHyp; ++i) {
        ran = i + 1;
        const int f = flags[(size_t)k * kHypPad + i];
        if (f == kFitNan) { st = SDFR_NOCS_NAN_INPUT; break; }
        if (f == kFitZeroVariance) { st = SDFR_NOCS_POSE_ERROR; break; }
        if (residual[i] < best) { best = residual[i]; winner = i; }
        if (best < stop_t) break;
      }
    }
    sel[0] = winner; sel[1] = ran; sel[2] = st;
  }
  __syncthreads();
  const int winner = sel[0];
  int st = sel[2];
  // inliers of the winner: |d_n| < pass_t; every point when no iteration beat 1e10 (:113)
  double M[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) M[i] = winner >= 0 ? transforms[((size_t)k * kHypPad + winner) * 12 + i] : 0.0;
  const double pass_t = header[k].pass_t;
  double a[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) a[i] = 0.0;
  // pass 1: flags, the reference's count (inlier INDICES that are non-zero, :167-169), the sums of the centroids
  for (int i = tid; i < r.n; i += kBlock) {
    const D3 s = load_point(src, i), t = load_point(tgt, i);
    bool in = true;
    if (winner >= 0) {
      const double dx = t.x - (M[0] * s.x + M[1] * s.y + M[2] * s.z + M[3]);
      const double dy = t.y - (M[4] * s.x + M[5] * s.y + M[6] * s.z + M[7]);
      const double dz = t.z - (M[8] * s.x + M[9] * s.y + M[10] * s.z + M[11]);
      in = sqrt(dx * dx + dy * dy + dz * dz) < pass_t;
    }
    inlier[r.begin + i] = in ? 1 : 0;
    if (inlier_mask) inlier_mask[r.begin + i] = in ? 1 : 0;
    if (in) {
      a[0] += 1.0;
      a[1] += (winner >= 0 && i != 0) ? 1.0 : 0.0;
      a[2] += s.x; a[3] += s.y; a[4] += s.z;
      a[5] += t.x; a[6] += t.y; a[7] += t.z;
    }
  }
  block_sum<8>(red, a);
  const double m = red[0][0];
  const double ratio = r.n > 0 ? red[1][0] / (double)r.n : 0.0;
  const D3 cs = d3(red[2][0] / m, red[3][0] / m, red[4][0] / m);
  const D3 ct = d3(red[5][0] / m, red[6][0] / m, red[7][0] / m);
  if (st == SDFR_NOCS_OK && ratio < 0.1) st = SDFR_NOCS_NONE;   // "Small inlier ratio" (:71-73)
  if (st == SDFR_NOCS_OK) {   // workgroup-uniform
    // pass 2: covariance and variance about the centroids
#pragma unroll
    for (int i = 0; i < 12; ++i) a[i] = 0.0;
    for (int i = tid; i < r.n; i += kBlock) {
      if (!inlier[r.begin + i]) continue;
      const D3 s = load_point(src, i), t = load_point(tgt, i);
      const D3 p = d3(t.x - ct.x, t.y - ct.y, t.z - ct.z);
      const D3 q = d3(s.x - cs.x, s.y - cs.y, s.z - cs.z);
      a[0] += p.x * q.x; a[1] += p.x * q.y; a[2] += p.x * q.z;
      a[3] += p.y * q.x; a[4] += p.y * q.y; a[5] += p.y * q.z;
      a[6] += p.z * q.x; a[7] += p.z * q.y; a[8] += p.z * q.z;
      a[9] += q.x * q.x; a[10] += q.y * q.y; a[11] += q.z * q.z;
    }
    block_sum<12>(red, a);
  }
  if (tid != 0) return;
  double T12[12], R[9], sc = qnan;
  if (st == SDFR_NOCS_OK) {
    double cov[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) cov[i] = red[i][0] / m;
    const double var = red[9][0] / m + red[10][0] / m + red[11][0] / m;
    const int f = umeyama_finish(cs, ct, cov, var, T12, R, &sc);
    if (f == kFitNan) st = SDFR_NOCS_NAN_INPUT;
    if (f == kFitZeroVariance) st = SDFR_NOCS_POSE_ERROR;
  }
  if (st != SDFR_NOCS_OK) {
#pragma unroll
    for (int i = 0; i < 12; ++i) T12[i] = qnan;
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = qnan;
    sc = qnan;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) position[3 * k + i] = T12[4 * i + 3];
#pragma unroll
  for (int i = 0; i < 9; ++i) rotation[9 * k + i] = R[i];
  scale[k] = sc;
#pragma unroll
  for (int i = 0; i < 12; ++i) transform[16 * k + i] = T12[i];
  const double zero = st == SDFR_NOCS_OK ? 0.0 : qnan;
  transform[16 * k + 12] = zero; transform[16 * k + 13] = zero; transform[16 * k + 14] = zero;
  transform[16 * k + 15] = st == SDFR_NOCS_OK ? 1.0 : qnan;
  inlier_ratio[k] = ratio;
  best_iteration[k] = winner;
  iterations_run[k] = sel[1];
  status[k] = st;
}

// grid K, kHypPad lanes: lane i draws row i
__global__ __launch_bounds__(kHypPad) void nocs_sample_kernel(const long long* __restrict__ offsets, int K,
                                                              unsigned long long seed,
                                                              const unsigned long long* __restrict__ seeds,
                                                              int* __restrict__ samples) {
  const int k = blockIdx.x, it = threadIdx.x;
  if (it >= kHyp) return;
  long long n64 = offsets[k + 1] - offsets[k];
  n64 = n64 < 0 ? 0 : (n64 > 0x7fffffffLL ? 0x7fffffffLL : n64);
  const unsigned n = (unsigned)n64;
  int* row = samples + ((size_t)k * kHyp + it) * 5;
  if (n < 5) {   // no five distinct indices exist; the fit answers SDFR_NOCS_NONE without reading them
    for (int d = 0; d < 5; ++d) row[d] = 0;
    return;
  }
  const unsigned long long key = seeds ? seeds[k] : seed;
  unsigned got[5];
  for (int d = 0; d < 5; ++d) {
    unsigned idx = 0;
    bool ok = false;
    for (int attempt = 0; attempt < kNocsMaxAttempts && !ok; ++attempt) {
      const U4 w = philox4x32_10(U4{(unsigned)it, (unsigned)d, (unsigned)attempt, kNocsStream}, (unsigned)key,
                                 (unsigned)(key >> 32));
      idx = (unsigned)(((unsigned long long)w.x * n) >> 32);
      ok = true;
      for (int e = 0; e < d; ++e) ok = ok && got[e] != idx;
    }
    if (!ok) {   // (4/5)^64 at worst: the smallest index not drawn yet
      for (idx = 0; idx < 5; ++idx) {
        bool used = false;
        for (int e = 0; e < d; ++e) used = used || got[e] == idx;
        if (!used) break;
      }
    }
    got[d] = idx;
    row[d] = (int)idx;
  }
}

int corr_check(const char* fn, int W, int H, int channels, int K) {
  if (W < 1 || H < 1 || (long long)W * H > 0x7fffffffLL - kCountPix)
    return fail(SDFR_E_INVALID, "%s: W=%d, H=%d invalid", fn, W, H);
  if (channels != 3 && channels != 4) return fail(SDFR_E_INVALID, "%s: channels=%d must be 3 or 4", fn, channels);
  if (K < 0 || K > 65535) return fail(SDFR_E_INVALID, "%s: K=%d out of range [0,65535]", fn, K);
  return 0;
}
inline int corr_blocks(int W, int H) { return (int)(((long long)W * H + kCountPix - 1) / kCountPix); }

int ransac_check(const char* fn, int K, long long total, int max_n) {
  if (K < 1 || K > 65535) return fail(SDFR_E_INVALID, "%s: K=%d out of range [1,65535]", fn, K);
  if (total < 0 || max_n < 0 || total < max_n)
    return fail(SDFR_E_INVALID, "%s: total=%lld, max_n=%d invalid (0 <= max_n <= total)", fn, total, max_n);
  return 0;
}
inline int ransac_chunks(int max_n) { return max_n > 0 ? (max_n + kEvalPts - 1) / kEvalPts : 1; }

struct FitLayout {
  size_t header, transforms, flags, partial, inlier, bytes;
};
FitLayout fit_layout(int K, long long total, int max_n) {
  FitLayout l;
  auto up = [](size_t x) { return (x + 127) & ~(size_t)127; };
  l.header = 0;
  l.transforms = up((size_t)K * sizeof(FitHeader));
  l.flags = l.transforms + (size_t)K * kHypPad * 12 * sizeof(double);
  l.partial = up(l.flags + (size_t)K * kHypPad * sizeof(int));
  l.inlier = l.partial + (size_t)K * ransac_chunks(max_n) * kHypPad * sizeof(double);
  l.bytes = up(l.inlier + (size_t)total);
  return l;
}

template <typename T>
void launch_fit(const void* source, const void* target, const long long* offsets, long long total, int max_n, int K,
                const int* samples, const FitLayout& l, char* ws, double* position, double* rotation, double* scale,
                double* transform, double* inlier_ratio, int* best_iteration, int* iterations_run, int* status,
                unsigned char* inlier_mask, hipStream_t st) {
  const T* s = (const T*)source;
  const T* t = (const T*)target;
  FitHeader* header = (FitHeader*)(ws + l.header);
  double* transforms = (double*)(ws + l.transforms);
  int* flags = (int*)(ws + l.flags);
  double* partial = (double*)(ws + l.partial);
  unsigned char* inlier = (unsigned char*)(ws + l.inlier);
  const int chunks = ransac_chunks(max_n);
  hipLaunchKernelGGL(ransac_hypotheses_kernel<T>, dim3(K), dim3(kBlock), 0, st, s, t, offsets, total, max_n, samples,
                     header, transforms, flags);
  hipLaunchKernelGGL(ransac_evaluate_kernel<T>, dim3(chunks, K), dim3(kHypPad), 0, st, s, t, offsets, total, max_n,
                     chunks, (const double*)transforms, partial);
  hipLaunchKernelGGL(ransac_finish_kernel<T>, dim3(K), dim3(kBlock), 0, st, s, t, offsets, total, max_n, chunks,
                     (const FitHeader*)header, (const double*)transforms, (const int*)flags, (const double*)partial,
                     inlier, position, rotation, scale, transform, inlier_ratio, best_iteration, iterations_run,
                     status, inlier_mask);
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_nocs_workspace_bytes(int W, int H, int K) {
  if (corr_check("sdfr_nocs_workspace_bytes", W, H, 3, K)) return 0;
  return (size_t)(K > 0 ? K : 1) * corr_blocks(W, H) * 8;
}

extern "C" int sdfr_nocs_count(const float* depth, const unsigned char* mask, int W, int H, const int* mask_ids, int K,
                               int* counts, float* max_depth, void* workspace, size_t workspace_bytes, int device,
                               void* stream) {
  if (int rc = corr_check("sdfr_nocs_count", W, H, 3, K)) return rc;
  if (K == 0) return 0;
  if (!depth || !mask || !mask_ids || !counts || !max_depth || !workspace)
    return fail(SDFR_E_NULL, "sdfr_nocs_count: NULL pointer argument");
  const size_t need = sdfr_nocs_workspace_bytes(W, H, K);
  if (workspace_bytes < need)
    return fail(SDFR_E_WORKSPACE, "sdfr_nocs_count: workspace %zu < %zu bytes", workspace_bytes, need);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int nblk = corr_blocks(W, H);
  int* bc = (int*)workspace;
  float* bm = (float*)workspace + (size_t)K * nblk;
  hipLaunchKernelGGL(nocs_count_kernel, dim3(nblk, K), dim3(kBlock), 0, st, depth, mask, W * H, mask_ids, nblk, bc, bm);
  hipLaunchKernelGGL(nocs_count_reduce_kernel, dim3(K), dim3(64), 0, st, (const int*)bc, (const float*)bm, nblk, counts,
                     max_depth);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_nocs_correspondences(const float* depth, const unsigned char* mask, const unsigned char* nocs,
                                         int channels, int W, int H, float rfx, float rfy, float cx0, float cy0,
                                         const int* mask_ids, int K, const long long* offsets, long long capacity,
                                         const void* workspace, float* source, float* target, int device,
                                         void* stream) {
  if (int rc = corr_check("sdfr_nocs_correspondences", W, H, channels, K)) return rc;
  if (capacity < 0) return fail(SDFR_E_INVALID, "sdfr_nocs_correspondences: capacity=%lld is negative", capacity);
  if (K == 0) return 0;
  if (!depth || !mask || !nocs || !mask_ids || !offsets || !workspace || !source || !target)
    return fail(SDFR_E_NULL, "sdfr_nocs_correspondences: NULL pointer argument");
  SDFR_HIP_TRY(hipSetDevice(device));
  const int nblk = corr_blocks(W, H);
  hipLaunchKernelGGL(nocs_compact_kernel, dim3(nblk, K), dim3(kBlock), 0, (hipStream_t)stream, depth, mask, nocs,
                     channels, W, W * H, mask_ids, nblk, (const int*)workspace, offsets, capacity, rfx, rfy, cx0, cy0,
                     source, target);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" size_t sdfr_similarity_ransac_workspace_bytes(int K, long long total, int max_n) {
  if (ransac_check("sdfr_similarity_ransac_workspace_bytes", K, total, max_n)) return 0;
  return fit_layout(K, total, max_n).bytes;
}

extern "C" int sdfr_similarity_ransac(const void* source, const void* target, int dtype, const long long* offsets,
                                      long long total, int max_n, int K, const int* sample_indices, double* position,
                                      double* rotation, double* scale, double* transform, double* inlier_ratio,
                                      int* best_iteration, int* iterations_run, int* status,
                                      unsigned char* inlier_mask, void* workspace, size_t workspace_bytes, int device,
                                      void* stream) {
  if (int rc = ransac_check("sdfr_similarity_ransac", K, total, max_n)) return rc;
  if (dtype != SDFR_NOCS_F32 && dtype != SDFR_NOCS_F64)
    return fail(SDFR_E_INVALID, "sdfr_similarity_ransac: dtype=%d must be SDFR_NOCS_F32 or SDFR_NOCS_F64", dtype);
  if ((total > 0 && (!source || !target)) || !offsets || !sample_indices || !position || !rotation || !scale ||
      !transform || !inlier_ratio || !best_iteration || !iterations_run || !status || !workspace)
    return fail(SDFR_E_NULL, "sdfr_similarity_ransac: NULL pointer argument (only inlier_mask may be NULL)");
  const FitLayout l = fit_layout(K, total, max_n);
  if (workspace_bytes < l.bytes)
    return fail(SDFR_E_WORKSPACE, "sdfr_similarity_ransac: workspace %zu < %zu bytes", workspace_bytes, l.bytes);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SDFR_NOCS_F32)
    launch_fit<float>(source, target, offsets, total, max_n, K, sample_indices, l, (char*)workspace, position, rotation,
                      scale, transform, inlier_ratio, best_iteration, iterations_run, status, inlier_mask, st);
  else
    launch_fit<double>(source, target, offsets, total, max_n, K, sample_indices, l, (char*)workspace, position,
                       rotation, scale, transform, inlier_ratio, best_iteration, iterations_run, status, inlier_mask,
                       st);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_nocs_sample_indices(const long long* offsets, int K, unsigned long long seed,
                                        const unsigned long long* object_seeds, int* sample_indices, int device,
                                        void* stream) {
  if (K < 0 || K > 65535) return fail(SDFR_E_INVALID, "sdfr_nocs_sample_indices: K=%d out of range [0,65535]", K);
  if (K == 0) return 0;
  if (!offsets || !sample_indices) return fail(SDFR_E_NULL, "sdfr_nocs_sample_indices: NULL pointer argument");
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(nocs_sample_kernel, dim3(K), dim3(kHypPad), 0, (hipStream_t)stream, offsets, K, seed,
                     object_seeds, sample_indices);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
