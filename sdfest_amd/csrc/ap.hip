// ap.hip -- detection matching and average precision, gfx950 (include/sdfr.h group 16): sdfr_pose_pair_errors,
// sdfr_ap_match, sdfr_ap_integrate.  All fp64, on the caller's stream, no allocation, no host synchronisation, and every
// sum in one fixed order: two calls on the same inputs give the same bits.
//
// THE PROTOCOL (the project's own statement, after the published NOCS evaluation; no parity with a third-party script
// is claimed.  tests/ap_twin.py says the same in numpy loops).
//   Groups.    Detections and ground truths carry a frame id and a class id; a GROUP is one (frame, class) and only
//              members of one group can match.
//   Order.     Inside a group the detections are processed by descending score, ties by the lower input index.
//   Pairs.     Every (detection i, ground truth j) of a group has four doubles: 0 iou, 1 degrees, 2 distance (metres),
//              3 key, the preference among ground truths.
//   Criterion. (iou_min, degrees_max, distance_max); a pair is ADMISSIBLE iff iou >= iou_min && degrees <= degrees_max
//              && distance <= distance_max.  -inf / +inf switch a test off; a pair with a NaN entry (the key included)
//              is never admissible.
//   Matching.  Criteria are independent of each other.  For one criterion, in detection order, a detection takes the
//              admissible, still unmatched ground truth with the smallest key (ties: the lower ground-truth index), or
//              stays unmatched.  key = -iou with (t, +inf, +inf) is the usual IoU matching, key = degrees + 100 distance
//              with (-inf, d, s) the usual degree / cm matching.
//   AP.        For one (class, criterion): all detections of the class over all frames by descending score (ties: the
//              lower input index), tp_k = detection k is matched, n_gt = the class's ground truths;
//                  precision_k = cumtp_k / (k + 1),  p^_k = max_{j >= k} precision_j,  AP = (sum_{k: tp_k} p^_k) / n_gt
//              -- the sum first, then one division: all matched gives exactly 1, none matched exactly 0.  n_gt == 0: NaN;
//              ground truths without detections: 0.  mAP is the mean over the classes whose AP is not NaN (host side).
//   Errors.    distance = |p_a - p_b|; degrees = 2 atan2(|v|, |w|) of the relative unit quaternion (v, w) -- q and -q
//              give the same value --, or with a symmetry axis a in {0, 1, 2} atan2(|a1 x a2|, a1 . a2) of the two images
//              of that object axis.  atan2, not acos: acos loses half the digits near 0 and 180 degrees.
//
// sdfr_ap_match: one thread per (group, criterion); a workgroup is one group and kMatchThreads consecutive criteria.  The
// loops over detections and ground truths have trip counts taken from the group, the same for every lane, and select
// without a branch; every lane reads the SAME table entry, so the loads have wave-uniform addresses and go through the
// scalar cache -- the table does not pass through LDS: a group's table is nd x ng x 32 bytes (1 152 bytes for 6 x 6),
// read once per wave from a cache that holds it, and staging it would add a barrier for nothing.  The matched set is one
// 64-bit mask per thread.
// sdfr_ap_integrate: one wave per (criterion, class): count the matches, then walk the class's slice from its end in
// chunks of 64 with the running maximum of the precision; a lane adds its terms in walk order and one xor butterfly adds
// the lanes.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "common.hpp"

namespace sdfr {
namespace {

constexpr int kPairThreads = 256;
constexpr int kMatchThreads = SDFR_AP_CRITERIA_BLOCK;   // criteria per workgroup
constexpr int kMatchMaxGt = SDFR_AP_MAX_GT;             // the matched set is one 64-bit mask
constexpr int kMaxCriteria = 1 << 20;
constexpr int kMaxGroups = 1 << 24;
constexpr unsigned char kUnmatched = SDFR_AP_UNMATCHED;
static_assert(kMatchMaxGt == 64 && kMatchThreads % 64 == 0, "one 64-bit mask; whole waves of criteria");

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// ---- pair errors ----------------------------------------------------------------------------------------------------
// No contraction here: x y - y x has to be exactly 0 for equal poses, and a fused multiply-add would leave the rounding
// error of one product.
__global__ void __launch_bounds__(kPairThreads) pose_pair_errors_kernel(const double* __restrict__ pose_a,
                                                                        const double* __restrict__ pose_b,
                                                                        const int* __restrict__ symmetry_axis, int N,
                                                                        double* __restrict__ degrees,
                                                                        double* __restrict__ distance) {
#pragma clang fp contract(off)
  const int n = blockIdx.x * kPairThreads + threadIdx.x;
  if (n >= N) return;
  double a[7], b[7];
  bool ok = true;
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    a[q] = pose_a[7 * (size_t)n + q], b[q] = pose_b[7 * (size_t)n + q];
    ok = ok && isfinite(a[q]) && isfinite(b[q]);
  }
  const int axis = symmetry_axis ? symmetry_axis[n] : -1;
  const double na = (a[3] * a[3] + a[4] * a[4]) + (a[5] * a[5] + a[6] * a[6]);
  const double nb = (b[3] * b[3] + b[4] * b[4]) + (b[5] * b[5] + b[6] * b[6]);
  ok = ok && na > 0.0 && nb > 0.0 && isfinite(na) && isfinite(nb);
  if (!ok) {
    degrees[n] = quiet_nan(), distance[n] = quiet_nan();
    return;
  }
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  distance[n] = sqrt(dx * dx + dy * dy + dz * dz);
  const double ia = 1.0 / sqrt(na), ib = 1.0 / sqrt(nb);
  const double ax = a[3] * ia, ay = a[4] * ia, az = a[5] * ia, aw = a[6] * ia;
  const double bx = b[3] * ib, by = b[4] * ib, bz = b[5] * ib, bw = b[6] * ib;
  const double to_degrees = 180.0 / 3.141592653589793238462643383279502884;
  double rad;
  if (axis >= 0 && axis <= 2) {
    // column `axis` of R(q): the image of that object axis
    double ux, uy, uz, vx, vy, vz;
    if (axis == 0) {
      ux = 1.0 - 2.0 * (ay * ay + az * az), uy = 2.0 * (ax * ay + az * aw), uz = 2.0 * (ax * az - ay * aw);
      vx = 1.0 - 2.0 * (by * by + bz * bz), vy = 2.0 * (bx * by + bz * bw), vz = 2.0 * (bx * bz - by * bw);
    } else if (axis == 1) {
      ux = 2.0 * (ax * ay - az * aw), uy = 1.0 - 2.0 * (ax * ax + az * az), uz = 2.0 * (ay * az + ax * aw);
      vx = 2.0 * (bx * by - bz * bw), vy = 1.0 - 2.0 * (bx * bx + bz * bz), vz = 2.0 * (by * bz + bx * bw);
    } else {
      ux = 2.0 * (ax * az + ay * aw), uy = 2.0 * (ay * az - ax * aw), uz = 1.0 - 2.0 * (ax * ax + ay * ay);
      vx = 2.0 * (bx * bz + by * bw), vy = 2.0 * (by * bz - bx * bw), vz = 1.0 - 2.0 * (bx * bx + by * by);
    }
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    rad = atan2(sqrt(cx * cx + cy * cy + cz * cz), ux * vx + uy * vy + uz * vz);
  } else {
    // a * conj(b), each difference of two products written so that equal quaternions cancel exactly
    const double rx = (ax * bw - aw * bx) + (az * by - ay * bz);
    const double ry = (ay * bw - aw * by) + (ax * bz - az * bx);
    const double rz = (az * bw - aw * bz) + (ay * bx - ax * by);
    const double rw = (aw * bw + ax * bx) + (ay * by + az * bz);
    rad = 2.0 * atan2(sqrt(rx * rx + ry * ry + rz * rz), fabs(rw));
  }
  degrees[n] = rad * to_degrees;
}

// ---- matching -------------------------------------------------------------------------------------------------------
// grid (G, ceil(T / kMatchThreads)).  A group whose offsets do not describe nd detections, ng <= 64 ground truths and
// nd x ng pairs inside the three buffers gets kUnmatched in its rows (where those lie inside [0, P)) and bit 0 of status.
__global__ void __launch_bounds__(kMatchThreads) ap_match_kernel(const double* __restrict__ table, long long n_pairs,
                                                                 const int* __restrict__ pred_offset,
                                                                 const int* __restrict__ gt_offset,
                                                                 const long long* __restrict__ pair_offset, int P,
                                                                 const double* __restrict__ criteria, int T,
                                                                 unsigned char* __restrict__ matched,
                                                                 int* __restrict__ status) {
  const int g = blockIdx.x;
  const int t = blockIdx.y * kMatchThreads + threadIdx.x;
  // (everything read here has a workgroup-uniform address)
  const int p0 = pred_offset[g], p1 = pred_offset[g + 1];
  const int g0 = gt_offset[g], g1 = gt_offset[g + 1];
  const long long e0 = pair_offset[g], e1 = pair_offset[g + 1];
  const bool rows_ok = p0 >= 0 && p1 >= p0 && p1 <= P;
  const long long nd = rows_ok ? (long long)p1 - p0 : 0;
  const long long ng = (long long)g1 - g0;
  const bool ok = rows_ok && g0 >= 0 && ng >= 0 && ng <= kMatchMaxGt && e0 >= 0 && e1 >= e0 && e1 <= n_pairs &&
                  e1 - e0 == nd * ng;
  if (!ok) {
    if (status && threadIdx.x == 0 && blockIdx.y == 0) atomicOr(status, 1);
    if (t < T)
      for (long long i = 0; i < nd; ++i) matched[(size_t)t * P + p0 + i] = kUnmatched;
    return;
  }
  const bool live = t < T;
  const int tc = live ? t : T - 1;   // lanes past T run along on the last criterion and write nothing
  const double iou_min = criteria[3 * (size_t)tc], degrees_max = criteria[3 * (size_t)tc + 1],
               distance_max = criteria[3 * (size_t)tc + 2];
  unsigned long long taken = 0ull;
  const int n_gt = (int)ng;
  const double* __restrict__ row = table + 4 * e0;
  for (int i = 0; i < (int)nd; ++i, row += 4 * n_gt) {
    double best_key = 0.0;
    int best = kUnmatched;
    for (int j = 0; j < n_gt; ++j) {
      const double iou = row[4 * j], deg = row[4 * j + 1], dist = row[4 * j + 2], key = row[4 * j + 3];
      // (comparisons with a NaN are false: a NaN entry is never admissible; key == key refuses a NaN key)
      const bool admissible = iou >= iou_min && deg <= degrees_max && dist <= distance_max && key == key &&
                              !((taken >> j) & 1ull);
      const bool take = admissible && (best == kUnmatched || key < best_key);
      best_key = take ? key : best_key;
      best = take ? j : best;
    }
    taken |= best == kUnmatched ? 0ull : 1ull << best;
    if (live) matched[(size_t)t * P + p0 + i] = (unsigned char)best;
  }
}

// ---- the AP integral ------------------------------------------------------------------------------------------------
// grid T * C workgroups of one wave: workgroup t * C + c.  The walk is bound by the latency of its two dependent loads
// (order, then the byte of `matched`): the flags of kIntegrateChunks chunks are fetched together before the chunks are
// taken one by one, and the count before the walk keeps four loads per lane in flight.
constexpr int kIntegrateChunks = 4;
__global__ void __launch_bounds__(64) ap_integrate_kernel(const unsigned char* __restrict__ matched, int T, int P,
                                                          const int* __restrict__ order,
                                                          const int* __restrict__ class_offset,
                                                          const int* __restrict__ n_gt, int C,
                                                          double* __restrict__ ap) {
  const int t = blockIdx.x / C, c = blockIdx.x % C;
  const int lane = threadIdx.x;
  const int o0 = class_offset[c], o1 = class_offset[c + 1];
  const int gts = n_gt[c];
  if (gts <= 0 || o0 < 0 || o1 < o0 || o1 > P) {   // uniform
    if (lane == 0) ap[(size_t)t * C + c] = quiet_nan();
    return;
  }
  const int n = o1 - o0;
  if (n == 0) {   // uniform: ground truths but no detections
    if (lane == 0) ap[(size_t)t * C + c] = 0.0;
    return;
  }
  const unsigned char* __restrict__ row = matched + (size_t)t * P;
  const int chunks = (n + 63) >> 6;
  // Is detection k of the slice matched?  Without a branch, so that the loads of several chunks can be in flight
  // together: the slot is clamped into the slice and the column into [0, P) (n >= 1, hence P >= 1), and what was clamped
  // does not count -- a detection index outside [0, P) counts as unmatched.
  auto is_tp = [&](int k) -> bool {
    const int slot = k < 0 ? 0 : (k < n ? k : n - 1);
    const int d = order[o0 + slot];
    const int col = d < 0 ? 0 : (d < P ? d : P - 1);
    return (row[col] != kUnmatched) & (k == slot) & (d == col);
  };
  int count = 0;
#pragma unroll 4
  for (int k = lane; k < 64 * chunks; k += 64) count += is_tp(k) ? 1 : 0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) count += __shfl_xor(count, d, 64);
  int before = count;   // matches in [0, 64 * (chunk + 1)) while walking down
  double sum = 0.0, envelope = 0.0;   // this lane's terms in walk order; precisions are >= 0
  for (int top = chunks - 1; top >= 0; top -= kIntegrateChunks) {
    bool tps[kIntegrateChunks];
#pragma unroll
    for (int u = 0; u < kIntegrateChunks; ++u) tps[u] = is_tp(64 * (top - u) + lane);   // (a chunk below 0: no slot, no match)
#pragma unroll
    for (int u = 0; u < kIntegrateChunks; ++u) {
      const int k = 64 * (top - u) + lane;
      const bool tp = tps[u];
      const unsigned long long m = __ballot(tp);
      before -= __popcll(m);
      const int cum = before + __popcll(m & (~0ull >> (63 - lane)));   // inclusive
      double p = k >= 0 && k < n ? (double)cum / (double)(k + 1) : 0.0;
      // suffix maximum over the chunk, then over the later chunks
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_down(p, d, 64);
        p = lane + d < 64 ? fmax(p, o) : p;
      }
      p = fmax(p, envelope);
      envelope = __shfl(p, 0, 64);
      sum += tp ? p : 0.0;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
  if (lane == 0) ap[(size_t)t * C + c] = sum / (double)gts;
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" int sdfr_pose_pair_errors(const double* pose_a, const double* pose_b, const int* symmetry_axis, int N,
                                     double* degrees, double* distance, int device, void* stream) {
  const char* fn = "sdfr_pose_pair_errors";
  if (N < 0) return fail(SDFR_E_INVALID, "%s: N=%d must be >= 0", fn, N);
  if (N == 0) return 0;
  if (!pose_a || !pose_b || !degrees || !distance)
    return fail(SDFR_E_NULL, "%s: NULL pointer argument (only symmetry_axis may be NULL)", fn);
  if (((uintptr_t)pose_a | (uintptr_t)pose_b | (uintptr_t)degrees | (uintptr_t)distance) & 7u)
    return fail(SDFR_E_INVALID, "%s: the poses and the outputs must be 8-byte aligned", fn);
  if ((uintptr_t)symmetry_axis & 3u) return fail(SDFR_E_INVALID, "%s: symmetry_axis must be 4-byte aligned", fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(pose_pair_errors_kernel, dim3((unsigned)((N + kPairThreads - 1) / kPairThreads)),
                     dim3(kPairThreads), 0, (hipStream_t)stream, pose_a, pose_b, symmetry_axis, N, degrees, distance);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_ap_match(const double* table, long long n_pairs, const int* pred_offset, const int* gt_offset,
                             const long long* pair_offset, int G, int P, const double* criteria, int T,
                             unsigned char* matched, int* status, int device, void* stream) {
  const char* fn = "sdfr_ap_match";
  if (n_pairs < 0 || G < 0 || P < 0 || T < 0)
    return fail(SDFR_E_INVALID, "%s: n_pairs=%lld, G=%d, P=%d, T=%d must be >= 0", fn, n_pairs, G, P, T);
  if (G > kMaxGroups) return fail(SDFR_E_INVALID, "%s: G=%d out of range [0,%d]", fn, G, kMaxGroups);
  if (T > kMaxCriteria) return fail(SDFR_E_INVALID, "%s: T=%d out of range [0,%d]", fn, T, kMaxCriteria);
  if (G == 0 || T == 0 || P == 0) return 0;
  if (!pred_offset || !gt_offset || !pair_offset || !criteria || !matched || (n_pairs > 0 && !table))
    return fail(SDFR_E_NULL, "%s: NULL pointer argument (only status may be NULL, and table when n_pairs is 0)", fn);
  if (((uintptr_t)table | (uintptr_t)pair_offset | (uintptr_t)criteria) & 7u)
    return fail(SDFR_E_INVALID, "%s: table, pair_offset and criteria must be 8-byte aligned", fn);
  if (((uintptr_t)pred_offset | (uintptr_t)gt_offset | (uintptr_t)status) & 3u)
    return fail(SDFR_E_INVALID, "%s: pred_offset, gt_offset and status must be 4-byte aligned", fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  if (status) zero_words_async(reinterpret_cast<float*>(status), 1, st);   // overwritten, never accumulated
  hipLaunchKernelGGL(ap_match_kernel, dim3((unsigned)G, (unsigned)((T + kMatchThreads - 1) / kMatchThreads)),
                     dim3(kMatchThreads), 0, st, table, n_pairs, pred_offset, gt_offset, pair_offset, P, criteria, T,
                     matched, status);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_ap_integrate(const unsigned char* matched, int T, int P, const int* order,
                                 const int* class_offset, const int* n_gt, int C, double* ap, int device,
                                 void* stream) {
  const char* fn = "sdfr_ap_integrate";
  if (T < 0 || P < 0 || C < 0) return fail(SDFR_E_INVALID, "%s: T=%d, P=%d, C=%d must be >= 0", fn, T, P, C);
  if (T > kMaxCriteria) return fail(SDFR_E_INVALID, "%s: T=%d out of range [0,%d]", fn, T, kMaxCriteria);
  if ((long long)T * C > INT_MAX)
    return fail(SDFR_E_INVALID, "%s: T=%d criteria x C=%d classes exceed an int32 count", fn, T, C);
  if (T == 0 || C == 0) return 0;
  if (!class_offset || !n_gt || !ap || (P > 0 && (!matched || !order)))
    return fail(SDFR_E_NULL, "%s: NULL pointer argument (matched and order may be NULL only when P is 0)", fn);
  if ((uintptr_t)ap & 7u) return fail(SDFR_E_INVALID, "%s: ap must be 8-byte aligned", fn);
  if (((uintptr_t)order | (uintptr_t)class_offset | (uintptr_t)n_gt) & 3u)
    return fail(SDFR_E_INVALID, "%s: order, class_offset and n_gt must be 4-byte aligned", fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(ap_integrate_kernel, dim3((unsigned)(T * C)), dim3(64), 0, (hipStream_t)stream, matched, T, P,
                     order, class_offset, n_gt, C, ap);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
