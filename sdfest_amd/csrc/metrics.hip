// metrics.hip -- surface sampling and exact nearest / farthest neighbours for reconstruction metrics, gfx950.
//
// What the reference's evaluation does on the CPU (rendering_evaluation.py:266-305): open3d's
// sample_points_uniformly on the estimated and the ground-truth mesh, then scipy KDTree queries inside
// sdfest/estimation/metrics.py.  Here:
//
// Sampling (sdfr_sample_points), K meshes in one launch sequence:
//   1. sample_area_kernel  (F_max / 256, K) -- |(b - a) x (c - a)| in fp64 from the fp32 unscaled vertices
//   2. sample_scan_kernel  (K)              -- inclusive scan of the areas, one workgroup per mesh, in a fixed order
//   3. sample_points_kernel(n / 256, K)     -- Philox-4x32-10 (key = seed, counter = sample index): two words give a
//                                              53-bit u, triangle = first t with cdf[t] > u cdf[F - 1] (binary search:
//                                              zero-area triangles are never chosen); r1, r2 from one word each,
//                                              open3d's barycentrics (1 - sqrt r1, sqrt r1 (1 - r2), sqrt r1 r2), then
//                                              scale, rotation and position
//   A mesh's samples depend on its own record, n and the seed only: a batch equals its single calls bit for bit.
//
// Neighbours (sdfr_nn_query), K pairs (query set k against reference set k, ragged through offsets[K + 1]):
//   1. nn_kernel   (ceil(max_q / 1024), slices, K) -- 256 lanes x 4 queries in registers; the workgroup's slice of the
//                  reference set passes through LDS as 16-byte records that every lane reads at the same address (a
//                  broadcast ds_read_b128); the fp32 norm sum decides, ties to the lowest reference index; the
//                  workgroup's winners merge into one 64-bit key per query with a vector atomicMin / atomicMax on
//                  (float bits << 32 | index) -- non-negative float bits order as unsigned integers, so the merged
//                  result is the same whatever the slicing or the arrival order (no float atomics)
//   2. nn_finalize_kernel (total_q / 256)      -- the chosen pair's distance again in fp64, and the index
// sdfr_nn_reduce: one workgroup per pair, a fixed-order fp64 tree over the pair's distances: sum, max, counts below
// thresholds (strict <), and below thresholds after dividing by a per-pair extent -- one read-back for every metric.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.hpp"
#include "philox.hpp"
#include "mesh_record.hpp"

// the CPU twin (tests/metrics_twin.py) evaluates every expression in this file operation by operation
#pragma clang fp contract(off)

namespace sdfr {
namespace {

constexpr int kSampleThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kNNThreads = 256;
constexpr int kNNQueriesPerLane = 4;
constexpr int kNNQueriesPerBlock = kNNThreads * kNNQueriesPerLane;
constexpr int kNNTile = 1024;             // reference points per LDS tile (16 KiB)
constexpr int kNNMinSlice = 256;          // reference points per workgroup, at least
constexpr int kNNTargetBlocks = 1024;     // the slicing aims at this many workgroups (4 per CU)
constexpr int kReduceThreads = 256;

// the record's face count, or 0 when its CDF range would leave the workspace (such a mesh's samples are NaN): the
// sampler's own rule, not mesh_record_faces -- it guards the workspace; the pointers are the caller's to keep valid
__device__ __forceinline__ int sample_faces(const sdfr_sample_mesh& m, long long total_faces, int max_faces) {
  const bool ok = m.num_faces >= 1 && m.num_faces <= max_faces && m.cdf_offset >= 0 &&
                  m.cdf_offset + m.num_faces <= total_faces;
  return ok ? m.num_faces : 0;
}

__device__ __forceinline__ V3 quat_rotate(const float* q, V3 v) {
  // v + 2 w (u x v) + 2 u x (u x v), u = (x, y, z): the form of pipeline.quaternion_apply
  const V3 u = mk(q[0], q[1], q[2]);
  const V3 t = cross(u, v);
  const V3 t2 = cross(u, t);
  return mk(v.x + 2.0f * (q[3] * t.x + t2.x), v.y + 2.0f * (q[3] * t.y + t2.y), v.z + 2.0f * (q[3] * t.z + t2.z));
}

__device__ __forceinline__ V3 load3(const float* __restrict__ p, long long i) {
  return mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
}

// the face's three vertex indices; false if one is negative (the caller also checks them against the vertex count)
__device__ __forceinline__ bool load_face(const int* __restrict__ f, long long t, int& a, int& b, int& c) {
  a = f[3 * t], b = f[3 * t + 1], c = f[3 * t + 2];
  return a >= 0 && b >= 0 && c >= 0;
}

__global__ void __launch_bounds__(kSampleThreads) sample_area_kernel(const sdfr_sample_mesh* __restrict__ meshes,
                                                                      long long total_faces, int max_faces,
                                                                      double* __restrict__ cdf) {
  const sdfr_sample_mesh m = meshes[blockIdx.y];
  const long long t = (long long)blockIdx.x * kSampleThreads + threadIdx.x;
  if (t >= sample_faces(m, total_faces, max_faces)) return;
  int a, b, c;
  double area = 0.0;
  if (load_face(m.faces, t, a, b, c) && a < m.num_vertices && b < m.num_vertices && c < m.num_vertices) {
    const V3 A = load3(m.vertices, a), B = load3(m.vertices, b), C = load3(m.vertices, c);
    const double ux = (double)B.x - (double)A.x, uy = (double)B.y - (double)A.y, uz = (double)B.z - (double)A.z;
    const double vx = (double)C.x - (double)A.x, vy = (double)C.y - (double)A.y, vz = (double)C.z - (double)A.z;
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    area = sqrt(cx * cx + cy * cy + cz * cz);
  }
  cdf[m.cdf_offset + t] = area;
}

// one workgroup per mesh: cdf := inclusive scan of the areas; each pass of kScanThreads elements is a wave scan, the
// waves' totals in order, the running carry -- the order of every addition depends on the face count alone
__global__ void __launch_bounds__(kScanThreads) sample_scan_kernel(const sdfr_sample_mesh* __restrict__ meshes,
                                                                    long long total_faces, int max_faces,
                                                                    double* __restrict__ cdf) {
  const sdfr_sample_mesh m = meshes[blockIdx.x];
  const int F = sample_faces(m, total_faces, max_faces);
  double* __restrict__ c = cdf + (F ? m.cdf_offset : 0);
  constexpr int kWaves = kScanThreads / 64;
  __shared__ double s_w[kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double carry = 0.0;
  for (long long base = 0; base < F; base += kScanThreads) {
    const long long t = base + threadIdx.x;
    double x = t < F ? c[t] : 0.0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    double off = carry, tot = carry;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) off += s_w[w];
      tot += s_w[w];
    }
    __syncthreads();
    if (t < F) c[t] = off + x;
    carry = tot;
  }
}

__global__ void __launch_bounds__(kSampleThreads) sample_points_kernel(const sdfr_sample_mesh* __restrict__ meshes,
                                                                        long long total_faces, int max_faces,
                                                                        const double* __restrict__ cdf, int n,
                                                                        unsigned k0, unsigned k1,
                                                                        float* __restrict__ points,
                                                                        float* __restrict__ normals,
                                                                        int* __restrict__ triangles) {
  const int k = blockIdx.y;
  const sdfr_sample_mesh m = meshes[k];
  const int i = blockIdx.x * kSampleThreads + threadIdx.x;
  if (i >= n) return;
  const long long row = (long long)k * n + i;
  const U4 r = philox4x32_10(U4{(unsigned)i, 0u, 0u, 0u}, k0, k1);
  const double u = ((double)(r.x >> 5) * 67108864.0 + (double)(r.y >> 6)) * (1.0 / 9007199254740992.0);
  const float r1 = (float)(r.z >> 8) * (1.0f / 16777216.0f);
  const float r2 = (float)(r.w >> 8) * (1.0f / 16777216.0f);
  const int F = sample_faces(m, total_faces, max_faces);
  const double* __restrict__ c = cdf + (F ? m.cdf_offset : 0);
  const double total = F ? c[F - 1] : 0.0;
  double target = u * total;
  if (!(target < total)) target = nextafter(total, 0.0);   // u < 1, but u * total may round up to total
  int lo = 0, hi = F ? F - 1 : 0;                           // first t with c[t] > target: c[F - 1] > target
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c[mid] > target) hi = mid;
    else lo = mid + 1;
  }
  const int t = lo;
  int a, b, cc;
  V3 P = mk(NAN, NAN, NAN), N = mk(NAN, NAN, NAN);
  // a face with an index outside the vertex array has area 0 and is never chosen unless every face has area 0
  // (total = 0): its samples are NaN
  const bool ok = total > 0.0 && load_face(m.faces, t, a, b, cc) && a < m.num_vertices && b < m.num_vertices &&
                  cc < m.num_vertices;
  if (ok) {
    const float s = sqrtf(r1);
    const float wa = 1.0f - s, wb = s * (1.0f - r2), wc = s * r2;
    const V3 A = load3(m.vertices, a), B = load3(m.vertices, b), C = load3(m.vertices, cc);
    P = mk(wa * A.x + wb * B.x + wc * C.x, wa * A.y + wb * B.y + wc * C.y, wa * A.z + wb * B.z + wc * C.z);
    P = quat_rotate(m.quat, m.factor * P);
    P = mk(P.x + m.position[0], P.y + m.position[1], P.z + m.position[2]);
    if (normals && m.normals) {
      const V3 NA = load3(m.normals, a), NB = load3(m.normals, b), NC = load3(m.normals, cc);
      N = mk(wa * NA.x + wb * NB.x + wc * NC.x, wa * NA.y + wb * NB.y + wc * NC.y, wa * NA.z + wb * NB.z + wc * NC.z);
      N = quat_rotate(m.quat, N);
      const float len = sqrtf(N.x * N.x + N.y * N.y + N.z * N.z);
      const float inv = len > 0.0f ? 1.0f / len : 0.0f;
      N = inv * N;
    }
  }
  points[3 * row] = P.x;
  points[3 * row + 1] = P.y;
  points[3 * row + 2] = P.z;
  if (normals) {
    normals[3 * row] = N.x;
    normals[3 * row + 1] = N.y;
    normals[3 * row + 2] = N.z;
  }
  if (triangles) triangles[row] = ok ? t : -1;
}

// ---- neighbours -----------------------------------------------------------------------------------------------------
enum NormKind { kL1 = 0, kL2 = 1, kLInf = 2, kLP = 3 };

// the fp32 quantity that decides: sum |d_i|^p (p = 2: squares, no root), max |d_i| for p = inf
template <int kNorm>
__device__ __forceinline__ float nn_key(float dx, float dy, float dz, float p) {
  if constexpr (kNorm == kL2) return dx * dx + dy * dy + dz * dz;
  if constexpr (kNorm == kL1) return fabsf(dx) + fabsf(dy) + fabsf(dz);
  if constexpr (kNorm == kLInf) return fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz));
  return powf(fabsf(dx), p) + powf(fabsf(dy), p) + powf(fabsf(dz), p);
}

// [lo, hi) of pair k, clamped to [0, total] (garbage offsets cannot read out of bounds)
__device__ __forceinline__ void nn_range(const long long* __restrict__ off, int k, long long total, long long& lo,
                                         long long& hi) {
  lo = min(max(off[k], 0LL), total);
  hi = min(max(off[k + 1], lo), total);
}

template <int kNorm, bool kFar>
__global__ void __launch_bounds__(kNNThreads) nn_kernel(const float* __restrict__ qpts,
                                                         const long long* __restrict__ qoff, long long total_q,
                                                         const float* __restrict__ rpts,
                                                         const long long* __restrict__ roff, long long total_r,
                                                         int slice, float p, unsigned long long* __restrict__ keys) {
  const int k = blockIdx.z;
  long long q0, q1, r0, r1;
  nn_range(qoff, k, total_q, q0, q1);
  nn_range(roff, k, total_r, r0, r1);
  const long long qb = (long long)blockIdx.x * kNNQueriesPerBlock;
  const long long rs = (long long)blockIdx.y * slice;
  if (qb >= q1 - q0 || rs >= r1 - r0) return;   // uniform over the workgroup
  const long long re = min(rs + slice, r1 - r0);

  float qx[kNNQueriesPerLane], qy[kNNQueriesPerLane], qz[kNNQueriesPerLane], best[kNNQueriesPerLane];
  int bi[kNNQueriesPerLane];
#pragma unroll
  for (int j = 0; j < kNNQueriesPerLane; ++j) {
    const long long q = qb + threadIdx.x + j * kNNThreads;
    const bool in = q < q1 - q0;
    const V3 v = in ? load3(qpts, q0 + q) : mk(0.f, 0.f, 0.f);
    qx[j] = v.x, qy[j] = v.y, qz[j] = v.z;
    best[j] = kFar ? -1.0f : INFINITY;
    bi[j] = -1;
  }

  __shared__ float4 s_ref[kNNTile];
  for (long long tb = rs; tb < re; tb += kNNTile) {
    const int tn = (int)min((long long)kNNTile, re - tb);
    __syncthreads();   // the previous tile is no longer read
    for (int t = threadIdx.x; t < tn; t += kNNThreads) {
      const V3 v = load3(rpts, r0 + tb + t);
      s_ref[t] = make_float4(v.x, v.y, v.z, __int_as_float((int)(tb + t)));   // w: the point's index in its set
    }
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < tn; ++t) {
      const float4 c = s_ref[t];   // the same address in every lane: one broadcast ds_read_b128
#pragma unroll
      for (int j = 0; j < kNNQueriesPerLane; ++j) {
        const float d = nn_key<kNorm>(qx[j] - c.x, qy[j] - c.y, qz[j] - c.z, p);
        // strict: the first (lowest) index keeps a tie; NaN never wins
        const bool better = kFar ? d > best[j] : d < best[j];
        best[j] = better ? d : best[j];
        bi[j] = better ? __float_as_int(c.w) : bi[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kNNQueriesPerLane; ++j) {
    const long long q = qb + threadIdx.x + j * kNNThreads;
    if (q >= q1 - q0 || bi[j] < 0) continue;
    // nearest: min over (bits, index) -> the lowest index among equal keys; farthest: max over (bits, ~index) -> the
    // same.  +0.0 and every positive float order as their bit patterns; -0.0 cannot occur (sums of |x|, x x)
    const unsigned long long bits = (unsigned long long)__float_as_uint(best[j]) << 32;
    unsigned long long* dst = keys + q0 + q;
    if (kFar)
      atomicMax(dst, bits | (unsigned)~(unsigned)bi[j]);
    else
      atomicMin(dst, bits | (unsigned)bi[j]);
  }
}

template <int kNorm>
__device__ __forceinline__ double nn_dist64(V3 a, V3 b, double p) {
  const double dx = fabs((double)a.x - (double)b.x), dy = fabs((double)a.y - (double)b.y),
               dz = fabs((double)a.z - (double)b.z);
  if constexpr (kNorm == kL2) return sqrt(dx * dx + dy * dy + dz * dz);
  if constexpr (kNorm == kL1) return dx + dy + dz;
  if constexpr (kNorm == kLInf) return fmax(fmax(dx, dy), dz);
  return pow(pow(dx, p) + pow(dy, p) + pow(dz, p), 1.0 / p);
}

template <int kNorm, bool kFar>
__global__ void __launch_bounds__(kSampleThreads) nn_finalize_kernel(const float* __restrict__ qpts,
                                                                      const long long* __restrict__ qoff,
                                                                      long long total_q,
                                                                      const float* __restrict__ rpts,
                                                                      const long long* __restrict__ roff,
                                                                      long long total_r, int K, double p,
                                                                      const unsigned long long* __restrict__ keys,
                                                                      double* __restrict__ dist,
                                                                      int* __restrict__ index) {
  const long long q = (long long)blockIdx.x * kSampleThreads + threadIdx.x;
  if (q >= total_q) return;
  // the pair of query q: the last k with qoff[k] <= q (binary search over the clamped offsets)
  int lo = 0, hi = K - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    long long a, b;
    nn_range(qoff, mid, total_q, a, b);
    if (a <= q) lo = mid;
    else hi = mid - 1;
  }
  long long q0, q1, r0, r1;
  nn_range(qoff, lo, total_q, q0, q1);
  nn_range(roff, lo, total_r, r0, r1);
  const unsigned long long key = keys[q];
  const unsigned idx = kFar ? ~(unsigned)key : (unsigned)key;
  if (q < q0 || q >= q1 || (long long)idx >= r1 - r0) {   // no reference point won (empty set, or NaN throughout)
    dist[q] = NAN;
    if (index) index[q] = -1;
    return;
  }
  dist[q] = nn_dist64<kNorm>(load3(qpts, q), load3(rpts, r0 + idx), p);
  if (index) index[q] = (int)idx;
}

// one workgroup per pair: stats[k] = {sum, max, n, #nan, count(d < t_j) j < 4, count(d / extent[k] < t_j) j < 4}
struct Thresholds {
  double t[SDFR_NN_MAX_THRESHOLDS];
  int n;
};

__global__ void __launch_bounds__(kReduceThreads) nn_reduce_kernel(const double* __restrict__ dist,
                                                                    const long long* __restrict__ off,
                                                                    long long total, Thresholds th,
                                                                    const double* __restrict__ extent,
                                                                    double* __restrict__ stats) {
  constexpr int kT = SDFR_NN_MAX_THRESHOLDS;
  const int k = blockIdx.x;
  long long lo, hi;
  nn_range(off, k, total, lo, hi);
  const double ext = extent ? extent[k] : 1.0;
  // thread partials over i = lo + tid, lo + tid + kReduceThreads, ..., then a halving tree in LDS: fixed order
  double acc[SDFR_NN_STATS];
#pragma unroll
  for (int j = 0; j < SDFR_NN_STATS; ++j) acc[j] = 0.0;
  for (long long i = lo + threadIdx.x; i < hi; i += kReduceThreads) {
    const double d = dist[i];
    if (!(d == d)) {
      acc[3] += 1.0;
      continue;
    }
    acc[0] += d;
    acc[1] = fmax(acc[1], d);
    acc[2] += 1.0;
    const double dn = d / ext;
#pragma unroll
    for (int j = 0; j < kT; ++j) {
      if (j < th.n && d < th.t[j]) acc[4 + j] += 1.0;
      if (j < th.n && dn < th.t[j]) acc[4 + kT + j] += 1.0;
    }
  }
  __shared__ double s[SDFR_NN_STATS][kReduceThreads];
#pragma unroll
  for (int j = 0; j < SDFR_NN_STATS; ++j) s[j][threadIdx.x] = acc[j];
  __syncthreads();
  for (int h = kReduceThreads / 2; h >= 1; h >>= 1) {
    if (threadIdx.x < h) {
#pragma unroll
      for (int j = 0; j < SDFR_NN_STATS; ++j) {
        const double o = s[j][threadIdx.x + h];
        s[j][threadIdx.x] = j == 1 ? fmax(s[j][threadIdx.x], o) : s[j][threadIdx.x] + o;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < SDFR_NN_STATS) stats[(size_t)k * SDFR_NN_STATS + threadIdx.x] = s[threadIdx.x][0];
}

template <int kNorm, bool kFar>
void nn_launch(const float* q, const long long* qoff, long long total_q, int max_q, const float* r,
               const long long* roff, long long total_r, int max_r, int K, float p, double* dist, int* index,
               unsigned long long* keys, hipStream_t st) {
  const int qblk = (max_q + kNNQueriesPerBlock - 1) / kNNQueriesPerBlock;
  // slices: enough workgroups for the chip (kNNTargetBlocks), none shorter than kNNMinSlice reference points
  const long long want = ((long long)kNNTargetBlocks + (long long)qblk * K - 1) / ((long long)qblk * K);
  long long slice = (max_r + want - 1) / want;
  slice = ((slice + 63) / 64) * 64;
  if (slice < kNNMinSlice) slice = kNNMinSlice;
  if ((max_r + slice - 1) / slice > 65535) slice = (max_r + 65534) / 65535;   // the grid's y extent
  const int nslice = (int)((max_r + slice - 1) / slice);
  hipLaunchKernelGGL((nn_kernel<kNorm, kFar>), dim3(qblk, nslice, K), dim3(kNNThreads), 0, st, q, qoff, total_q, r,
                     roff, total_r, (int)slice, p, keys);
  hipLaunchKernelGGL((nn_finalize_kernel<kNorm, kFar>), dim3((unsigned)((total_q + kSampleThreads - 1) / kSampleThreads)),
                     dim3(kSampleThreads), 0, st, q, qoff, total_q, r, roff, total_r, K, (double)p,
                     (const unsigned long long*)keys, dist, index);
}

template <bool kFar>
void nn_dispatch(float p, const float* q, const long long* qoff, long long total_q, int max_q, const float* r,
                 const long long* roff, long long total_r, int max_r, int K, double* dist, int* index,
                 unsigned long long* keys, hipStream_t st) {
  if (p == 1.0f)
    nn_launch<kL1, kFar>(q, qoff, total_q, max_q, r, roff, total_r, max_r, K, p, dist, index, keys, st);
  else if (p == 2.0f)
    nn_launch<kL2, kFar>(q, qoff, total_q, max_q, r, roff, total_r, max_r, K, p, dist, index, keys, st);
  else if (std::isinf(p))
    nn_launch<kLInf, kFar>(q, qoff, total_q, max_q, r, roff, total_r, max_r, K, p, dist, index, keys, st);
  else
    nn_launch<kLP, kFar>(q, qoff, total_q, max_q, r, roff, total_r, max_r, K, p, dist, index, keys, st);
}

inline int nn_check(const char* fn, int K, long long total_q, int max_q, long long total_r, int max_r) {
  if (K < 1 || K > 65535) return fail(SDFR_E_INVALID, "%s: K=%d out of range [1,65535]", fn, K);
  if (max_q < 1 || total_q < max_q)
    return fail(SDFR_E_INVALID, "%s: max_q=%d must be in [1,total_q=%lld]", fn, max_q, total_q);
  if (max_r < 1 || total_r < max_r)
    return fail(SDFR_E_INVALID, "%s: max_r=%d must be in [1,total_r=%lld]", fn, max_r, total_r);
  if (total_r > 0x7fffffffLL) return fail(SDFR_E_INVALID, "%s: total_r=%lld exceeds 2^31-1", fn, total_r);
  return 0;
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_sample_workspace_bytes(int K, long long total_faces, int max_faces) {
  if (mesh_table_check("sdfr_sample_workspace_bytes", K, total_faces, max_faces)) return 0;
  return (size_t)total_faces * sizeof(double);
}

extern "C" int sdfr_sample_points(const sdfr_sample_mesh* meshes, int K, long long total_faces, int max_faces, int n,
                                  unsigned long long seed, float* points, float* normals, int* triangles,
                                  void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (int rc = mesh_table_check("sdfr_sample_points", K, total_faces, max_faces)) return rc;
  if (n < 1) return fail(SDFR_E_INVALID, "sdfr_sample_points: n=%d must be >= 1", n);
  if (!meshes || !points || !workspace)
    return fail(SDFR_E_NULL, "sdfr_sample_points: NULL pointer argument (only normals and triangles may be NULL)");
  const size_t need = sdfr_sample_workspace_bytes(K, total_faces, max_faces);
  if (workspace_bytes < need)
    return fail(SDFR_E_WORKSPACE, "sdfr_sample_points: workspace %zu < %zu bytes", workspace_bytes, need);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  double* cdf = (double*)workspace;
  hipLaunchKernelGGL(sample_area_kernel, dim3((max_faces + kSampleThreads - 1) / kSampleThreads, K),
                     dim3(kSampleThreads), 0, st, meshes, total_faces, max_faces, cdf);
  hipLaunchKernelGGL(sample_scan_kernel, dim3(K), dim3(kScanThreads), 0, st, meshes, total_faces, max_faces, cdf);
  hipLaunchKernelGGL(sample_points_kernel, dim3((n + kSampleThreads - 1) / kSampleThreads, K), dim3(kSampleThreads), 0,
                     st, meshes, total_faces, max_faces, (const double*)cdf, n, (unsigned)seed, (unsigned)(seed >> 32), points, normals,
                     triangles);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" size_t sdfr_nn_workspace_bytes(int K, long long total_q, int max_q) {
  if (K < 1 || max_q < 1 || total_q < max_q) {
    set_error("sdfr_nn_workspace_bytes: K=%d, total_q=%lld, max_q=%d invalid", K, total_q, max_q);
    return 0;
  }
  return (size_t)total_q * sizeof(unsigned long long);
}

extern "C" int sdfr_nn_query(const float* queries, const long long* q_offsets, long long total_q, int max_q,
                             const float* refs, const long long* r_offsets, long long total_r, int max_r, int K,
                             float p, int farthest, double* dist, int* index, void* workspace, size_t workspace_bytes,
                             int device, void* stream) {
  if (int rc = nn_check("sdfr_nn_query", K, total_q, max_q, total_r, max_r)) return rc;
  if (!(p >= 1.0f)) return fail(SDFR_E_INVALID, "sdfr_nn_query: p=%g must be >= 1 (inf allowed)", (double)p);
  if (farthest != 0 && farthest != 1)
    return fail(SDFR_E_INVALID, "sdfr_nn_query: farthest=%d must be 0 or 1", farthest);
  if (!queries || !q_offsets || !refs || !r_offsets || !dist || !workspace)
    return fail(SDFR_E_NULL, "sdfr_nn_query: NULL pointer argument (only index may be NULL)");
  const size_t need = (size_t)total_q * sizeof(unsigned long long);
  if (workspace_bytes < need)
    return fail(SDFR_E_WORKSPACE, "sdfr_nn_query: workspace %zu < %zu bytes", workspace_bytes, need);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  // nearest starts from all ones (above every key), farthest from zero (below every key)
  SDFR_HIP_TRY(hipMemsetAsync(keys, farthest ? 0x00 : 0xff, need, st));
  if (farthest)
    nn_dispatch<true>(p, queries, q_offsets, total_q, max_q, refs, r_offsets, total_r, max_r, K, dist, index, keys, st);
  else
    nn_dispatch<false>(p, queries, q_offsets, total_q, max_q, refs, r_offsets, total_r, max_r, K, dist, index, keys,
                       st);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_nn_reduce(const double* dist, const long long* offsets, long long total, int K,
                              const double* h_thresholds, int num_thresholds, const double* extent, double* stats,
                              int device, void* stream) {
  if (K < 1 || K > 65535) return fail(SDFR_E_INVALID, "sdfr_nn_reduce: K=%d out of range [1,65535]", K);
  if (total < 1) return fail(SDFR_E_INVALID, "sdfr_nn_reduce: total=%lld must be >= 1", total);
  if (num_thresholds < 0 || num_thresholds > SDFR_NN_MAX_THRESHOLDS)
    return fail(SDFR_E_INVALID, "sdfr_nn_reduce: num_thresholds=%d out of range [0,%d]", num_thresholds,
                SDFR_NN_MAX_THRESHOLDS);
  if (!dist || !offsets || !stats || (num_thresholds > 0 && !h_thresholds))
    return fail(SDFR_E_NULL, "sdfr_nn_reduce: NULL pointer argument (only extent may be NULL)");
  Thresholds th{};
  th.n = num_thresholds;
  for (int j = 0; j < num_thresholds; ++j) th.t[j] = h_thresholds[j];
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(nn_reduce_kernel, dim3(K), dim3(kReduceThreads), 0, (hipStream_t)stream, dist, offsets, total,
                     th, extent, stats);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
