// pc_information.hip -- Gauss-Newton information of the point-cloud residual (gfx950 only): sdfr_pc_information, and
// sdfr_information_combine, which adds it to the depth term's for sdfr_lm_step.
//
// Per view, the F x F Gram matrix, F = 10 + T, of the per-point feature vector f = (e0 .. e7, s0 .. s_{T-1}, r, 1) over
// ALL points of the view.  r is the point's value as sdfr_pc_loss_forward writes it (load_frame, sample_cell and trilerp
// of sampler_device.hpp, times scale; 0 outside the volume); e = d r / d (p, q, inv_scale) -- the expressions of
// pc_backward_block with upstream gradient 1, RESTATED here (that function is the captured loop's hot path and is not
// touched; tests/test_pc_information_gpu.py holds J^T r against sdfr_pc_loss_backward), the quaternion part through
// the normalisation per point and the scale part turned to group 14's coordinate, d / d inv_scale = -scale^2 d / d scale;
// s_t = scale * trilerp(jac[.][t]) at the point's cell with the point's offsets.  A point outside the volume is a member
// of the reference's mean with residual 0 and no gradient: f = (0, .., 0, 0, 1).
//
// The Gram product and the latent features are information_gram.hpp's, shared with render_information_shape_kernel: a
// wave's 64 points are the rows.
//
// The grid.  (min(nblk, G), B) workgroups of 256 points, G = kPcInfoGroups: workgroup g of a view takes the view's blocks
// g, g + G, g + 2 G, ... (as PcBackwardArgs::groups) and keeps its accumulators across them, so a view writes
// min(nb_v, G) records whatever the capacity of the point buffers is.  The stride is the CONSTANT G, not the grid's
// width: which points meet in one accumulator, and in which order, depends on the view's own points alone -- not on B,
// the other views or max_view_points.  A second launch sums a view's records in record order in double; how many there
// are follows from the offsets, so the workspace needs no flags and may hold anything on entry.
#include <cmath>

#include "common.hpp"
#include "device.hpp"
#include "information_gram.hpp"
#include "sampler_device.hpp"

namespace sdfr {
namespace {

// G: workgroups per view.  The longest fp32 chain is 64 ceil(nb_v / G) points (nb_v: the view's blocks).  64: a mug's ~60
// blocks of a 640 x 480 view are one block a workgroup (64 points a chain), a view whose every pixel is a point (1 200
// blocks) 19 (1 216, worst-case rounding 1 216 x 2^-24 = 7e-5 of sum |f_i f_j|, under the tests' 1e-4), and one view alone
// still starts 64 workgroups.  Here and not in tuning.hpp: that file holds what a variant build may override (and the
// benchmark ties its counter profile to its bytes); G decides which points share an accumulator and so the result's
// bits -- a build with another G would not compute what this one computes.
constexpr int kPcInfoGroups = 64;
// a workgroup's count, 256 ceil(nblk / G), must stay an exact float
constexpr long long kPcInfoMaxPoints = (long long)kPcInfoGroups << 24;
static_assert(kPts == 64 * kGramWaves, "one Gram block per wave");

// d value / d (p, q^, scale) of one inside point: pc_backward_block's acc[0 .. 7] with go = 1
template <int RT>
__device__ __forceinline__ void point_derivatives(const PointFrame& f, const Cell& c, int R, V3 vrel, V3 o, float tri,
                                                  float (&a)[8]) {
  const int Rr = RT > 0 ? RT : R;
  const float gsz = 2.0f / (float)(Rr - 1);  // grid size
  const float ax = 1.0f - c.ox, ay = 1.0f - c.oy, az = 1.0f - c.oz;
  const float c00 = fmaf(c.v[4], c.ox, c.v[0] * ax), c01 = fmaf(c.v[5], c.ox, c.v[1] * ax);
  const float c10 = fmaf(c.v[6], c.ox, c.v[2] * ax), c11 = fmaf(c.v[7], c.ox, c.v[3] * ax);
  V3 G;  // d tri / d (cell coordinate)
  G.x = ((c.v[4] - c.v[0]) * ay + (c.v[6] - c.v[2]) * c.oy) * az +
        ((c.v[5] - c.v[1]) * ay + (c.v[7] - c.v[3]) * c.oy) * c.oz;
  G.y = (c10 - c00) * az + (c11 - c01) * c.oz;
  G.z = fmaf(c11, c.oy, c01 * ay) - fmaf(c10, c.oy, c00 * ay);
  // value = tri(off) * scale, off = (o/scale - cellpos)/g  =>  d value / d o = G / g
  const V3 dvo = mk(G.x / gsz, G.y / gsz, G.z / gsz);
  // d value / d scale = tri - (dvo . o) / scale
  a[7] = tri - dot(dvo, o) / f.scale;
  // o = R^T (P - p): d/dp = -R dvo
  a[0] = -fmaf(f.rot[0], dvo.x, fmaf(f.rot[1], dvo.y, f.rot[2] * dvo.z));
  a[1] = -fmaf(f.rot[3], dvo.x, fmaf(f.rot[4], dvo.y, f.rot[5] * dvo.z));
  a[2] = -fmaf(f.rot[6], dvo.x, fmaf(f.rot[7], dvo.y, f.rot[8] * dvo.z));
  // R^T v = (1 - 2|u|^2) v + 2 u (u.v) - 2 w (u x v):
  //   d/du_k = -4 u_k v + 2 e_k (u.v) + 2 u v_k - 2 w (e_k x v),   d/dw = -2 (u x v)
  const V3 u = mk(f.qn[0], f.qn[1], f.qn[2]);
  const float w = f.qn[3];
  const float udv = dot(u, vrel), Dv = dot(dvo, vrel), Du = dot(dvo, u);
  const V3 vxD = cross(vrel, dvo);  // dvo . (e_k x v) = (v x dvo)_k
  a[3] = -4.0f * u.x * Dv + 2.0f * udv * dvo.x + 2.0f * vrel.x * Du - 2.0f * w * vxD.x;
  a[4] = -4.0f * u.y * Dv + 2.0f * udv * dvo.y + 2.0f * vrel.y * Du - 2.0f * w * vxD.y;
  a[5] = -4.0f * u.z * Dv + 2.0f * udv * dvo.z + 2.0f * vrel.z * Du - 2.0f * w * vxD.z;
  a[6] = -2.0f * dot(dvo, cross(u, vrel));
}

// grid: (min(nblk, G), B).  records [B][gridDim.x][F F], F = 10 + T; Tp = 0 with T = 0 (jac is not read).
template <int RT>
__global__ __launch_bounds__(kPts) void pc_information_kernel(
    const float* __restrict__ points, const int* __restrict__ offsets, int n_single, const float* __restrict__ pos,
    const float* __restrict__ quat, const float* __restrict__ scale, const float* __restrict__ sdf, int R,
    long long sdf_view_stride, const float* __restrict__ jac, int Tp, int T, long long jac_view_stride,
    float* __restrict__ records, int* __restrict__ inside) {
  __shared__ GramBlock lds[kGramWaves];
  __shared__ int lds_inside[kGramWaves];
  const int v = blockIdx.y, g = blockIdx.x;
  const int begin = offsets ? offsets[v] : 0;
  const int end = offsets ? offsets[v + 1] : n_single;
  const int len = end - begin;
  if ((long long)g * kPts >= len) return;   // no block of this view (workgroup-uniform): the reduce never reads its slot
  const int Rr = RT > 0 ? RT : R;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int F = 10 + T;
  const PointFrame fr = load_frame(pos, quat, scale, v);
  const float* vol = sdf + (size_t)v * sdf_view_stride;
  const float* jv = jac + (size_t)v * jac_view_stride;
  f32x16 acc;
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0f;
  int n_inside = 0;   // (wave-uniform)

#pragma unroll 1
  for (long long b = g; b * kPts < len; b += kPcInfoGroups) {   // (workgroup-uniform)
    const long long first = b * kPts + 64 * wave;   // the wave's first point of this block, relative to the view
    if (first >= len) continue;                     // wave-uniform: no rows, no products (all-zero rows add nothing)
    const long long rel = first + lane;
    float f[kGramF];
#pragma unroll
    for (int k = 0; k < kGramF; ++k) f[k] = 0.0f;
    bool live = false;
    if (rel < len) {
      const size_t i = (size_t)begin + (size_t)rel;
      const V3 P = mk(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
      V3 vrel, o;
      Cell c;
      live = sample_cell<RT>(fr, vol, R, P, vrel, o, c);
      float r = 0.0f;
      if (live) {
        const float tri = trilerp(c);
        float a[8];
        point_derivatives<RT>(fr, c, R, vrel, o, tri, a);
        f[0] = a[0]; f[1] = a[1]; f[2] = a[2];
        // q^ = q / |q|: what pc_loss_reduce_kernel applies to the summed partials, here per point
        const float d = fr.qn[0] * a[3] + fr.qn[1] * a[4] + fr.qn[2] * a[5] + fr.qn[3] * a[6];
#pragma unroll
        for (int k = 0; k < 4; ++k) f[3 + k] = (a[3 + k] - fr.qn[k] * d) * fr.inv_norm;
        f[7] = -(fr.scale * fr.scale) * a[7];   // d / d inv_scale
        if (T > 0) latent_features(c, jv, Tp, T, Rr, fr.scale, f);
        r = tri * fr.scale;
      }
#pragma unroll
      for (int k = 8; k < kGramF; ++k) f[k] = k == 8 + T ? r : k == 9 + T ? 1.0f : f[k];
    }
    n_inside += __popcll(__ballot(live));
    gram32_accumulate(f, lds[wave], lane, acc);
  }
  gram32_store(acc, lds[wave], lane);
  if (lane == 0) lds_inside[wave] = n_inside;
  __syncthreads();
  gram32_record(lds, F, tid, records + ((size_t)v * gridDim.x + g) * (size_t)(F * F));
  // (integers: whatever order the view's workgroups arrive in, the sum is the same)
  if (inside && tid == 0) atomicAdd(inside + v, (lds_inside[0] + lds_inside[1]) + (lds_inside[2] + lds_inside[3]));
}

// A view's min(nb_v, G) records summed in record order in double, one thread per entry.  grid: B; 256 threads.
__global__ __launch_bounds__(256) void pc_information_reduce_kernel(const float* __restrict__ records,
                                                                    const int* __restrict__ offsets, int n_single,
                                                                    int slots, int rec, double* __restrict__ gram) {
  const int v = blockIdx.x;
  const int len = offsets ? offsets[v + 1] - offsets[v] : n_single;
  const long long nb = len > 0 ? ((long long)len + kPts - 1) / kPts : 0;
  const int n = (int)(nb < slots ? nb : slots);
  const float* recs = records + (size_t)v * slots * rec;
  for (int e = threadIdx.x; e < rec; e += 256) {
    double a = 0.0;
    for (int t = 0; t < n; ++t) a += (double)recs[(size_t)t * rec + e];
    gram[(size_t)v * rec + e] = a;
  }
}

// sdfr_information_combine: workgroup k is object k.  IEEE double operations in the stated order, no fused multiply-add:
// a float64 restatement gives the same bits.
__global__ __launch_bounds__(256) void information_combine_kernel(const double* gd, const double* gp, int V, int F,
                                                                  double pc_weight, double* out) {
#pragma clang fp contract(off)
  const int k = blockIdx.x;
  const int rec = F * F, last = rec - 1;
  const double* d0 = gd + (size_t)k * V * rec;
  const double* p0 = gp + (size_t)k * V * rec;
  double* o0 = out + (size_t)k * V * rec;
  double cd = 0.0, cp = 0.0;
  for (int v = 0; v < V; ++v) {   // views ascending; every thread the same sums
    cd = cd + d0[(size_t)v * rec + last];
    cp = cp + p0[(size_t)v * rec + last];
  }
  const double alpha = (cd > 0.0 && cp > 0.0) ? (pc_weight * cd) / cp : 0.0;
  __syncthreads();   // (in place: the counts are read before anything is written)
  for (int e = threadIdx.x; e < V * rec; e += 256) {
    const int w = e % rec, i = w / F, j = w % F;
    const double d = d0[e];
    double r = d;
    if (i < F - 1 && j < F - 1) {
      const double prod = alpha * p0[e];
      r = d + prod;
    }
    o0[e] = r;
  }
}

inline int pc_info_slots(int max_view_points) {
  const long long nblk = ((long long)max_view_points + kPts - 1) / kPts;
  return (int)(nblk < kPcInfoGroups ? nblk : kPcInfoGroups);
}
inline bool pc_info_sizes_ok(int B, int max_view_points, int T) {
  return B >= 0 && B <= 65535 && max_view_points >= 0 && (long long)max_view_points <= kPcInfoMaxPoints && T >= 0 &&
         T <= SDFR_INFO_MAX_TANGENTS;
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_pc_information_workspace_bytes(int B, int max_view_points, int T) {
  if (!pc_info_sizes_ok(B, max_view_points, T)) return 0;
  return (size_t)B * pc_info_slots(max_view_points) * (size_t)((10 + T) * (10 + T)) * sizeof(float);
}

extern "C" int sdfr_pc_information(const float* points, const int* offsets, int B, int max_view_points,
                                   const float* pos, const float* quat, const float* scale, const float* sdf, int R,
                                   long long sdf_view_stride, const float* jac, int Tp, int T, long long jac_view_stride,
                                   double* gram, int* inside, void* workspace, size_t workspace_bytes, int device,
                                   void* stream) {
  const char* fn = "sdfr_pc_information";
  if (B < 0 || B > 65535) return fail(SDFR_E_INVALID, "%s: B=%d out of range [0,65535]", fn, B);
  if (max_view_points < 0 || (long long)max_view_points > kPcInfoMaxPoints)
    return fail(SDFR_E_INVALID, "%s: max_view_points=%d out of range [0,%lld]", fn, max_view_points, kPcInfoMaxPoints);
  if (R < 2 || R > 1024) return fail(SDFR_E_INVALID, "%s: R=%d out of range [2,1024]", fn, R);
  if (T < 0 || T > SDFR_INFO_MAX_TANGENTS)
    return fail(SDFR_E_INVALID, "%s: T=%d out of range [0,%d]", fn, T, SDFR_INFO_MAX_TANGENTS);
  if (T > 0 && (Tp < T || (Tp & 3)))
    return fail(SDFR_E_INVALID, "%s: Tp=%d must be a multiple of 4 and at least T=%d", fn, Tp, T);
  if (sdf_view_stride != 0 && sdf_view_stride < (long long)R * R * R)
    return fail(SDFR_E_INVALID, "%s: sdf_view_stride must be 0 or >= R^3", fn);
  if (T > 0 && jac_view_stride != 0 && jac_view_stride < (long long)R * R * R * Tp)
    return fail(SDFR_E_INVALID, "%s: jac_view_stride must be 0 or >= R^3 Tp", fn);
  if (!offsets && B > 1) return fail(SDFR_E_INVALID, "%s: offsets may be NULL only for a single view", fn);
  if (B == 0) return 0;
  if (!gram) return fail(SDFR_E_INVALID, "%s: NULL pointer argument (gram)", fn);
  if ((uintptr_t)gram & 7u) return fail(SDFR_E_INVALID, "%s: gram must be 8-byte aligned", fn);
  const int F = 10 + T, rec = F * F;
  if (max_view_points == 0) {
    SDFR_HIP_TRY(hipSetDevice(device));
    hipStream_t st0 = (hipStream_t)stream;
    zero_words_async((float*)gram, (size_t)B * rec * 2, st0);
    if (inside) zero_words_async((float*)inside, (size_t)B, st0);
    SDFR_HIP_TRY(hipGetLastError());
    return 0;
  }
  if (!points || !pos || !quat || !scale || !sdf || (T > 0 && !jac) || !workspace)
    return fail(SDFR_E_INVALID, "%s: NULL pointer argument", fn);
  const size_t need = sdfr_pc_information_workspace_bytes(B, max_view_points, T);
  if (workspace_bytes < need) return fail(SDFR_E_INVALID, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
  if (((uintptr_t)workspace & 127u) || (T > 0 && (((uintptr_t)jac & 15u) || (jac_view_stride & 3))))
    return fail(SDFR_E_INVALID, "%s: workspace must be 128-byte, jac (and its view stride) 16-byte and gram 8-byte aligned",
                fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int slots = pc_info_slots(max_view_points);
  float* records = (float*)workspace;
  if (inside) zero_words_async((float*)inside, (size_t)B, st);
  const dim3 grid((unsigned)slots, (unsigned)B);
  const float* jp = T > 0 ? jac : sdf;   // (never read with T = 0; a valid address for the view offset all the same)
  const int tp = T > 0 ? Tp : 0;
  const long long js = T > 0 ? jac_view_stride : 0;
  if (R == 64)
    hipLaunchKernelGGL((pc_information_kernel<64>), grid, dim3(kPts), 0, st, points, offsets, max_view_points, pos, quat,
                       scale, sdf, R, sdf_view_stride, jp, tp, T, js, records, inside);
  else
    hipLaunchKernelGGL((pc_information_kernel<0>), grid, dim3(kPts), 0, st, points, offsets, max_view_points, pos, quat,
                       scale, sdf, R, sdf_view_stride, jp, tp, T, js, records, inside);
  hipLaunchKernelGGL(pc_information_reduce_kernel, dim3((unsigned)B), dim3(256), 0, st, records, offsets,
                     max_view_points, slots, rec, gram);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_information_combine(const double* gram_depth, const double* gram_pc, int K, int V, int T,
                                        double pc_weight, double* gram_out, int device, void* stream) {
  const char* fn = "sdfr_information_combine";
  if (K < 1 || K > 65535 || V < 1 || V > SDFR_LM_MAX_VIEWS || T < 0 || T > SDFR_INFO_MAX_TANGENTS)
    return fail(SDFR_E_INVALID, "%s: K=%d, V=%d, T=%d: need 1 <= K <= 65535, 1 <= V <= %d, 0 <= T <= %d", fn, K, V, T,
                SDFR_LM_MAX_VIEWS, SDFR_INFO_MAX_TANGENTS);
  if (!(pc_weight >= 0.0) || !std::isfinite(pc_weight))
    return fail(SDFR_E_INVALID, "%s: pc_weight=%g must be finite and >= 0", fn, pc_weight);
  if (!gram_depth || !gram_pc || !gram_out) return fail(SDFR_E_INVALID, "%s: NULL pointer argument", fn);
  if (((uintptr_t)gram_depth & 7u) || ((uintptr_t)gram_pc & 7u) || ((uintptr_t)gram_out & 7u))
    return fail(SDFR_E_INVALID, "%s: the matrices must be 8-byte aligned", fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(information_combine_kernel, dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream, gram_depth,
                     gram_pc, V, 10 + T, pc_weight, gram_out);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
