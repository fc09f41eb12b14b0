// boxes.hip -- oriented bounding boxes, gfx950: the bounds of a grid's iso-surface without its mesh (sdfr_sdf_bounds)
// and the exact intersection volume of two oriented boxes (sdfr_box_iou).
//
// sdfr_sdf_bounds.  The bounds are the minimum and maximum, per axis, of the vertices sdfr_mesh_emit would place on the
// crossed edges of the same (padded) grid -- mesh_grid.hpp holds the one statement of which edges are crossed and
// where their vertices lie, so the two agree bit for bit.  Launch sequence on the caller's stream:
//   1. bounds_init_kernel      the N output rows := {+inf x 3, -inf x 3} as order-preserving integers, crossed := 0
//   2. bounds_reduce_kernel    (M^3 / 1024, N): every point's crossed owned edges -> wave -> workgroup -> one integer
//                              atomicMin / atomicMax per axis and one atomicAdd per workgroup that has a crossing
//   3. bounds_finish_kernel    the integers back to floats, in place
// Minimum, maximum and an integer sum do not depend on the order of their operands: the same bits every call, for a
// grid alone or among N.
//
// sdfr_box_iou.  The intersection of two boxes is a convex polytope whose faces lie on the 12 face planes, and with the
// origin at box a's centre its volume is (1/3) sum_f d_f area(f), d_f = the signed distance of face f's plane.  The face
// on a plane of box X is X's rectangle clipped against the other box's six half-spaces (Sutherland-Hodgman in the
// rectangle's own 2-D coordinates, at most 4 + 6 = 10 vertices).  Signed distances of at most 1e-12 L, L = |e_a| + |e_b|
// + |c_b - c_a|, count as zero, and a rectangle of b that lies entirely
// ON a plane of a with the same outward normal is dropped: a's own rectangle has counted that face.  One lane per (pair,
// symmetry step); the lanes of a pair share a wave-sized workgroup and lane 0 takes the largest volume in a fixed order.
// The polygons are indexed at run time and live in LDS, laid out [vertex][lane].
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "common.hpp"
#include "mesh_grid.hpp"

namespace sdfr {
namespace {

// ---- bounds ---------------------------------------------------------------------------------------------------------
constexpr int kBoundsThreads = 256;
constexpr int kBoundsPoints = 4;   // points per thread, kBoundsThreads apart

// a float as an int whose signed order is the float's (finite values and the infinities; -0 below +0)
__device__ __forceinline__ int ordered_int(float f) {
  const int b = __float_as_int(f);
  return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float ordered_float(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__global__ void bounds_init_kernel(int N, int* __restrict__ keys, int* __restrict__ crossed) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int lo = ordered_int(INFINITY), hi = ordered_int(-INFINITY);
  for (int a = 0; a < 3; ++a) keys[6 * n + a] = lo, keys[6 * n + 3 + a] = hi;
  crossed[n] = 0;
}

__global__ void bounds_finish_kernel(int N, int* __restrict__ keys) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= 6 * N) return;
  keys[q] = __float_as_int(ordered_float(keys[q]));
}

__global__ void __launch_bounds__(kBoundsThreads) bounds_reduce_kernel(MeshGrid p, float s, float h,
                                                                       int* __restrict__ keys,
                                                                       int* __restrict__ crossed) {
  const int n = blockIdx.y;
  const float* __restrict__ g = p.sdf + (size_t)n * p.R * p.R * p.R;
  const int M = p.M;
  const int pts = M * M * M;   // <= 258^3
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int count = 0;
#pragma unroll
  for (int r = 0; r < kBoundsPoints; ++r) {
    const int pt = (blockIdx.x * kBoundsPoints + r) * kBoundsThreads + threadIdx.x;
    if (pt >= pts) continue;
    const int i = pt / (M * M), j = pt / M % M, k = pt % M;
    const float v0 = mesh_at(g, p, i, j, k);
    const unsigned m = mesh_owned_edges(g, p, i, j, k, v0);
    if (!m) continue;
    count += __popc(m);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!(m & (1u << a))) continue;
      const float v1 = mesh_at(g, p, i + (a == 0), j + (a == 1), k + (a == 2));
      const V3 v = mesh_edge_vertex(i, j, k, a, mesh_edge_t(v0, v1, p.level), s, h);
      lo[0] = fminf(lo[0], v.x), lo[1] = fminf(lo[1], v.y), lo[2] = fminf(lo[2], v.z);
      hi[0] = fmaxf(hi[0], v.x), hi[1] = fmaxf(hi[1], v.y), hi[2] = fmaxf(hi[2], v.z);
    }
  }
  __shared__ float s_lo[kBoundsThreads / 64][3], s_hi[kBoundsThreads / 64][3];
  __shared__ int s_count[kBoundsThreads / 64];
  const int wave = threadIdx.x >> 6;
  if (__ballot(count != 0)) {   // most waves see no crossing: they skip the shuffles
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      count += __shfl_xor(count, d, 64);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = fminf(lo[a], __shfl_xor(lo[a], d, 64));
        hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d, 64));
      }
    }
  }
  if ((threadIdx.x & 63) == 0) {
    s_count[wave] = count;
#pragma unroll
    for (int a = 0; a < 3; ++a) s_lo[wave][a] = lo[a], s_hi[wave][a] = hi[a];
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < kBoundsThreads / 64; ++w) total += s_count[w];
    if (total == 0) return;
    const int q = threadIdx.x;
    if (q == 6) {
      atomicAdd(&crossed[n], total);
    } else if (q < 3) {
      float v = s_lo[0][q];
#pragma unroll
      for (int w = 1; w < kBoundsThreads / 64; ++w) v = fminf(v, s_lo[w][q]);
      atomicMin(&keys[6 * n + q], ordered_int(v));
    } else {
      float v = s_hi[0][q - 3];
#pragma unroll
      for (int w = 1; w < kBoundsThreads / 64; ++w) v = fmaxf(v, s_hi[w][q - 3]);
      atomicMax(&keys[6 * n + q], ordered_int(v));
    }
  }
}

// ---- box intersection -----------------------------------------------------------------------------------------------
constexpr int kIouLanes = 64;      // one wave per workgroup
constexpr int kIouVertices = 10;   // a rectangle clipped by six half-spaces
constexpr int kIouMaxSteps = 65536;
constexpr double kIouSnap = 1e-12;   // x L: a vertex this close to a plane is on it

struct D3 {
  double x, y, z;
};
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 operator*(double s, D3 a) { return D3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double norm(D3 a) { return sqrt(dot(a, a)); }

// centre, the three axes (columns of R(q)) and the half side lengths along them.  No arrays: the face loops below turn
// the axes cyclically instead of indexing them, so everything stays in registers.
struct Box {
  D3 c, a0, a1, a2;
  double h0, h1, h2;
};
__device__ __forceinline__ void turn(Box& b) {   // (axis 0, 1, 2) := (axis 1, 2, 0)
  const D3 a = b.a0;
  const double h = b.h0;
  b.a0 = b.a1, b.a1 = b.a2, b.a2 = a;
  b.h0 = b.h1, b.h1 = b.h2, b.h2 = h;
}

// the ten doubles of a box; false for a non-finite entry, a non-positive extent or a quaternion without a direction
__device__ __forceinline__ bool load_box(const double* __restrict__ r, Box& b, double& volume, double& diagonal) {
  double v[10];
  bool ok = true;
#pragma unroll
  for (int q = 0; q < 10; ++q) {
    v[q] = r[q];
    ok = ok && isfinite(v[q]);
  }
  const double n2 = v[3] * v[3] + v[4] * v[4] + v[5] * v[5] + v[6] * v[6];
  ok = ok && v[7] > 0.0 && v[8] > 0.0 && v[9] > 0.0 && n2 > 0.0 && isfinite(n2);
  if (!ok) return false;
  const double inv = 1.0 / sqrt(n2);
  const double x = v[3] * inv, y = v[4] * inv, z = v[5] * inv, w = v[6] * inv;
  b.c = D3{v[0], v[1], v[2]};
  b.a0 = D3{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y + z * w), 2.0 * (x * z - y * w)};
  b.a1 = D3{2.0 * (x * y - z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z + x * w)};
  b.a2 = D3{2.0 * (x * z + y * w), 2.0 * (y * z - x * w), 1.0 - 2.0 * (x * x + y * y)};
  b.h0 = 0.5 * v[7], b.h1 = 0.5 * v[8], b.h2 = 0.5 * v[9];
  volume = v[7] * v[8] * v[9];
  diagonal = norm(D3{v[7], v[8], v[9]});
  return true;
}

// the polygon in `src` (m vertices, (u, v) of vertex i at src[(2 i + {0, 1}) * kIouLanes]) clipped to c0 + ca u + cb v
// <= 0 into `dst`; returns the new vertex count.  A signed distance within `tol` counts as zero.  strict: a polygon that
// lies on the line altogether is dropped.
__device__ __forceinline__ int clip_polygon(const double* src, double* dst, double* dist, int m, double c0, double ca,
                                            double cb, double tol, bool strict) {
  bool all_on = true;
  for (int i = 0; i < m; ++i) {
    double s = c0 + ca * src[(2 * i) * kIouLanes] + cb * src[(2 * i + 1) * kIouLanes];
    if (fabs(s) <= tol) s = 0.0;
    dist[i * kIouLanes] = s;
    all_on = all_on && s == 0.0;
  }
  if (strict && all_on) return 0;
  int count = 0;
  for (int i = 0; i < m; ++i) {
    const int i1 = i + 1 == m ? 0 : i + 1;
    const double sa = dist[i * kIouLanes], sb = dist[i1 * kIouLanes];
    const double ua = src[(2 * i) * kIouLanes], va = src[(2 * i + 1) * kIouLanes];
    if (sa <= 0.0) {
      if (count < kIouVertices) dst[(2 * count) * kIouLanes] = ua, dst[(2 * count + 1) * kIouLanes] = va;
      ++count;
    }
    if ((sa < 0.0 && sb > 0.0) || (sa > 0.0 && sb < 0.0)) {
      const double ub = src[(2 * i1) * kIouLanes], vb = src[(2 * i1 + 1) * kIouLanes];
      const double t = sa / (sa - sb);
      if (count < kIouVertices)
        dst[(2 * count) * kIouLanes] = ua + t * (ub - ua), dst[(2 * count + 1) * kIouLanes] = va + t * (vb - va);
      ++count;
    }
  }
  return count < kIouVertices ? count : kIouVertices;
}

// sum over the six faces of `own` of d_f area(face clipped to `other`); strict: see clip_polygon.  Both boxes come back
// as they went in (three turns each).
__device__ __forceinline__ double faces_sum(Box& own, Box& other, bool strict, double tol, double* poly, double* dist) {
  double sum = 0.0;
#pragma unroll 1
  for (int k = 0; k < 3; ++k) {
#pragma unroll 1
    for (int sign = 0; sign < 2; ++sign) {
      const double sg = sign ? -1.0 : 1.0;
      const D3 n = sg * own.a0;
      const D3 centre = own.c + own.h0 * n;
      const double d = dot(n, own.c) + own.h0;
      // the rectangle's axes, ordered so that u x v = n
      const D3 u = sign ? own.a2 : own.a1, v = sign ? own.a1 : own.a2;
      const double hu = sign ? own.h2 : own.h1, hv = sign ? own.h1 : own.h2;
      double* src = poly;
      double* dst = poly + 2 * kIouVertices * kIouLanes;
      src[0 * kIouLanes] = -hu, src[1 * kIouLanes] = -hv;
      src[2 * kIouLanes] = hu, src[3 * kIouLanes] = -hv;
      src[4 * kIouLanes] = hu, src[5 * kIouLanes] = hv;
      src[6 * kIouLanes] = -hu, src[7 * kIouLanes] = hv;
      int m = 4;
#pragma unroll 1
      for (int j = 0; j < 6; ++j) {
        if (m >= 3) {
          const D3 nj = (j & 1) ? -1.0 * other.a0 : other.a0;
          const double dj = dot(nj, other.c) + other.h0;
          m = clip_polygon(src, dst, dist, m, dot(nj, centre) - dj, dot(nj, u), dot(nj, v), tol,
                           strict && dot(nj, n) > 0.0);
          double* t = src;
          src = dst, dst = t;
        }
        if (j & 1) turn(other);
      }
      if (m >= 3) {
        const double u0 = src[0], v0 = src[kIouLanes];
        double twice = 0.0;
        for (int i = 1; i + 1 < m; ++i) {
          const double ua = src[(2 * i) * kIouLanes] - u0, va = src[(2 * i + 1) * kIouLanes] - v0;
          const double ub = src[(2 * i + 2) * kIouLanes] - u0, vb = src[(2 * i + 3) * kIouLanes] - v0;
          twice += ua * vb - va * ub;
        }
        sum += d * (0.5 * twice);
      }
    }
    turn(own);
  }
  return sum;
}

__global__ void __launch_bounds__(kIouLanes) box_iou_kernel(const double* __restrict__ boxes_a,
                                                            const double* __restrict__ boxes_b, int M, int paired,
                                                            long long pairs, int axis, int steps, int group,
                                                            double* __restrict__ iou,
                                                            double* __restrict__ intersection) {
  __shared__ double s_poly[2 * 2 * kIouVertices * kIouLanes];
  __shared__ double s_dist[kIouVertices * kIouLanes];
  __shared__ double s_volume[kIouLanes];
  const int lane = threadIdx.x;
  const int per_block = kIouLanes / group;   // pairs per workgroup; `group` lanes share a pair's symmetry steps
  const int local = lane / group, member = lane % group;
  const long long pair = (long long)blockIdx.x * per_block + local;
  const bool active = local < per_block && pair < pairs;
  double best = 0.0, va = 0.0, vb = 0.0;
  bool valid = false;
  if (active) {
    const long long ia = paired ? pair : pair / M, ib = paired ? pair : pair % M;
    Box a, b;
    double da, db;
    const bool ok_a = load_box(boxes_a + 10 * ia, a, va, da);   // both are read whatever the first says
    const bool ok_b = load_box(boxes_b + 10 * ib, b, vb, db);
    valid = ok_a && ok_b;
    if (valid) {
      b.c = b.c - a.c;   // the origin at a's centre
      a.c = D3{0.0, 0.0, 0.0};
      const double apart = norm(b.c);
      // (bounding spheres apart: disjoint, exactly 0)
      if (!(apart > 0.5 * (da + db))) {
        const double tol = kIouSnap * (da + db + apart);
        double* poly = s_poly + lane;
        double* dist = s_dist + lane;
        for (int step = member; step < steps; step += group) {
          Box t = b;
          if (step) {   // b turned about its own axis by 2 pi step / steps (step 0: b as it is, the same bits)
            double sn, cs;
            sincospi(2.0 * (double)step / (double)steps, &sn, &cs);
            if (axis == 0) t.a1 = cs * b.a1 + sn * b.a2, t.a2 = cs * b.a2 - sn * b.a1;
            if (axis == 1) t.a2 = cs * b.a2 + sn * b.a0, t.a0 = cs * b.a0 - sn * b.a2;
            if (axis == 2) t.a0 = cs * b.a0 + sn * b.a1, t.a1 = cs * b.a1 - sn * b.a0;
          }
          double v = (faces_sum(a, t, false, tol, poly, dist) + faces_sum(t, a, true, tol, poly, dist)) * (1.0 / 3.0);
          v = fmin(fmax(v, 0.0), fmin(va, vb));
          best = fmax(best, v);
        }
      }
    }
  }
  if (group > 1) {
    s_volume[lane] = best;
    __syncthreads();
    if (active && member == 0)
      for (int g = 1; g < group; ++g) best = fmax(best, s_volume[lane + g]);
  }
  if (active && member == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    iou[pair] = valid ? best / (va + vb - best) : nan;
    if (intersection) intersection[pair] = valid ? best : nan;
  }
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" int sdfr_sdf_bounds(const float* sdf, int N, int R, int complete, float level, float* bounds, int* crossed,
                               int device, void* stream) {
  const char* fn = "sdfr_sdf_bounds";
  if (N < 0 || N > 65535) return fail(SDFR_E_INVALID, "%s: N=%d out of range [0,65535]", fn, N);
  if (R < 2 || R > 256) return fail(SDFR_E_INVALID, "%s: R=%d out of range [2,256]", fn, R);
  if (complete != 0 && complete != 1) return fail(SDFR_E_INVALID, "%s: complete=%d must be 0 or 1", fn, complete);
  if (!std::isfinite(level)) return fail(SDFR_E_INVALID, "%s: level=%g must be finite", fn, (double)level);
  if (N == 0) return 0;
  if (!sdf || !bounds || !crossed) return fail(SDFR_E_INVALID, "%s: NULL pointer argument", fn);
  if (((uintptr_t)bounds & 3u) || ((uintptr_t)crossed & 3u) || ((uintptr_t)sdf & 3u))
    return fail(SDFR_E_INVALID, "%s: sdf, bounds and crossed must be 4-byte aligned", fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int M = mesh_side(R, complete);
  const int per_block = kBoundsThreads * kBoundsPoints;
  const int nblk = (int)(((long long)M * M * M + per_block - 1) / per_block);
  const MeshGrid p{sdf, R, M, complete, level};
  int* keys = (int*)bounds;
  hipLaunchKernelGGL(bounds_init_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, keys, crossed);
  hipLaunchKernelGGL(bounds_reduce_kernel, dim3(nblk, N), dim3(kBoundsThreads), 0, st, p, mesh_vertex_scale(R),
                     mesh_vertex_half(M), keys, crossed);
  hipLaunchKernelGGL(bounds_finish_kernel, dim3((6 * N + 255) / 256), dim3(256), 0, st, N, keys);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_box_iou(const double* boxes_a, int N, const double* boxes_b, int M, int mode, int symmetry_axis,
                            int symmetry_steps, double* iou, double* intersection, int device, void* stream) {
  const char* fn = "sdfr_box_iou";
  if (N < 0 || M < 0) return fail(SDFR_E_INVALID, "%s: N=%d, M=%d must be >= 0", fn, N, M);
  if (mode != SDFR_BOX_IOU_MATRIX && mode != SDFR_BOX_IOU_PAIRED)
    return fail(SDFR_E_INVALID, "%s: mode=%d must be SDFR_BOX_IOU_MATRIX or SDFR_BOX_IOU_PAIRED", fn, mode);
  if (mode == SDFR_BOX_IOU_PAIRED && N != M)
    return fail(SDFR_E_INVALID, "%s: SDFR_BOX_IOU_PAIRED needs N == M (N=%d, M=%d)", fn, N, M);
  if (symmetry_axis < -1 || symmetry_axis > 2)
    return fail(SDFR_E_INVALID, "%s: symmetry_axis=%d must be -1, 0, 1 or 2", fn, symmetry_axis);
  if (symmetry_axis >= 0 && (symmetry_steps < 1 || symmetry_steps > kIouMaxSteps))
    return fail(SDFR_E_INVALID, "%s: symmetry_steps=%d out of range [1,%d]", fn, symmetry_steps, kIouMaxSteps);
  if (N == 0 || M == 0) return 0;
  if (!boxes_a || !boxes_b || !iou) return fail(SDFR_E_INVALID, "%s: NULL pointer argument (only intersection may be NULL)", fn);
  if (((uintptr_t)boxes_a & 7u) || ((uintptr_t)boxes_b & 7u) || ((uintptr_t)iou & 7u) || ((uintptr_t)intersection & 7u))
    return fail(SDFR_E_INVALID, "%s: the boxes and the outputs must be 8-byte aligned", fn);
  const int paired = mode == SDFR_BOX_IOU_PAIRED;
  const long long pairs = paired ? (long long)N : (long long)N * M;
  const int steps = symmetry_axis >= 0 ? symmetry_steps : 1;
  const int group = steps < kIouLanes ? steps : kIouLanes;
  const int per_block = kIouLanes / group;
  const long long blocks = (pairs + per_block - 1) / per_block;
  if (blocks > INT_MAX) return fail(SDFR_E_INVALID, "%s: %lld pairs with %d symmetry steps are too many", fn, pairs, steps);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(box_iou_kernel, dim3((unsigned)blocks), dim3(kIouLanes), 0, (hipStream_t)stream, boxes_a, boxes_b,
                     M, paired, pairs, symmetry_axis, steps, group, iou, intersection);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
