// information_shape.hip -- joint Gauss-Newton information of pose AND latent (gfx950 only): sdfr_render_information_shape.
//
// Per view, the F x F Gram matrix, F = 10 + T, of the per-pixel feature vector f = (d0 .. d7, s0 .. s_{T-1}, r, 1) over
// the included pixels.  d, r and the inclusion rule are sdfr_render_information's (information_device.hpp: the same
// hit_point, gather_cell, __fdiv_rn inlier test and tile cull).  s_t = d depth / d z_t: the backward's d depth / d SDF
// weights of a hit pixel are f * (the trilinear weights of its cell), f = scale |d.z| (render.hip, backward_tile, the
// SDFR_SDF_GRAD_EXACT branch), so s_t = f * trilerp(jac[.][t]) at the pixel's cell with the pixel's offsets -- eight
// more gathers of Tp floats at a point pixel_derivatives has already located (jac is voxel-major for this: the T
// tangents of a grid corner are Tp / 4 16-byte loads).
//
// The Gram product.  F <= 32, so one v_mfma_f32_32x32x2_f32 block holds it: lane l holds A[l & 31][l >> 5] and
// B[l >> 5][l & 31], and with A = F^T, B = F both are the SAME register, feature l & 31 of pixel 2 g + (l >> 5) of k-step
// g -- word 64 g + l of the wave's [pixel][32] block in LDS, 32 MFMAs per 64 pixels into 16 accumulator registers.  The
// alternative, three 16 x 16 x 4 products on a low and a high half of the features (low x low, low x high, high x high),
// would issue 48 MFMAs of half the cycles per 64 pixels -- three quarters of the matrix-core time -- but needs two
// operand reads per step, three accumulators and the low x high block mirrored by hand to keep (i, j) and (j, i) the
// same bits.  The kernel's time is expected in the 8 (1 + Tp) gathered floats per hit pixel, not in 32 MFMAs per
// sub-tile (supposed, not measured in advance), so the form with one read, one instruction and one layout per step is
// the one built.  As in information.hip the instruction is a k-ordered fma chain: one order, symmetric bit for bit, an
// excluded pixel's row all zeros, entry (F - 1, F - 1) the exact count.
//
// Two launches, as sdfr_render_information: the tile kernel over all views (a tile without an included pixel writes a 0
// flag and nothing else), then a fixed-order sum of each view's tile records in double.
#include <cmath>

#include "information_device.hpp"

namespace sdfr {
namespace {

constexpr int kShapeMaxT = 22;       // 10 + T <= 32
constexpr int kShapeF = 32;          // feature slots of a pixel's row
constexpr int kShapeChunks = 8;      // the reduce kernel: chunks of a view's tiles summed side by side
constexpr int kShapeLanes = 128;     // ... by this many threads each, 128 entries of the record per pass

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ShapeLds {
  // per wave: [pixel][feature], features F .. 31 zero; the wave's 32 x 32 block (row-major) overlays it at the end
  float feat[kInfoBlock / 64][64 * kShapeF];
};

// the T latent features of one hit pixel into f[8 ..]: the cell is gather_cell's (the same clamped floor of the same
// hit point), the blend trilerp's (x, then y, then z)
template <int RT>
__device__ __forceinline__ void latent_features(const ViewSetup& s, const float* __restrict__ jac, int Tp, int T, int R,
                                                int row, int col, float z, float cx, float cy, float rfx, float rfy,
                                                float (&f)[kShapeF]) {
  const int Rr = RT > 0 ? RT : R;
  const float h = 0.5f * (float)(Rr - 1);
  const HitPoint hp = hit_point(s, row, col, z, cx, cy, rfx, rfy, s.isc, h);
  const float top = (float)(Rr - 2);
  const float bx = fminf(fmaxf(floorf(hp.gx), 0.0f), top);
  const float by = fminf(fmaxf(floorf(hp.gy), 0.0f), top);
  const float bz = fminf(fmaxf(floorf(hp.gz), 0.0f), top);
  const float ox = hp.gx - bx, oy = hp.gy - by, oz = hp.gz - bz;
  const float ax = 1.0f - ox, ay = 1.0f - oy, az = 1.0f - oz;
  const int lin = (Rr <= 256) ? (int)fmaf(fmaf(bx, (float)Rr, by), (float)Rr, bz)
                              : ((int)bx * Rr + (int)by) * Rr + (int)bz;
  const float fw = s.scale * fabsf(hp.d.z);
  const float* base = jac + (size_t)lin * Tp;
  const size_t sy = (size_t)Rr * Tp, sx = (size_t)Rr * Rr * Tp;
#pragma unroll
  for (int g = 0; g < (kShapeMaxT + 3) / 4; ++g) {
    if (4 * g >= Tp) continue;   // wave-uniform
    const float* p = base + 4 * g;
    // corner 4 ix + 2 iy + iz, as Cell::v
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(p), v1 = *reinterpret_cast<const f32x4*>(p + Tp);
    const f32x4 v2 = *reinterpret_cast<const f32x4*>(p + sy), v3 = *reinterpret_cast<const f32x4*>(p + sy + Tp);
    const f32x4 v4 = *reinterpret_cast<const f32x4*>(p + sx), v5 = *reinterpret_cast<const f32x4*>(p + sx + Tp);
    const f32x4 v6 = *reinterpret_cast<const f32x4*>(p + sx + sy), v7 = *reinterpret_cast<const f32x4*>(p + sx + sy + Tp);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float c00 = fmaf(v4[j], ox, v0[j] * ax), c01 = fmaf(v5[j], ox, v1[j] * ax);
      const float c10 = fmaf(v6[j], ox, v2[j] * ax), c11 = fmaf(v7[j], ox, v3[j] * ax);
      const float c0 = fmaf(c10, oy, c00 * ay), c1 = fmaf(c11, oy, c01 * ay);
      const float tri = fmaf(c1, oz, c0 * az);
      if (8 + 4 * g + j < kShapeF) f[8 + 4 * g + j] = 4 * g + j < T ? fw * tri : 0.0f;
    }
  }
}

// grid: (tiles in x, tiles in y, B).  flags [B][tiles]: 1 = the tile has a record; records [B][tiles][F F], F = 10 + T.
template <int RT>
__global__ __launch_bounds__(kInfoBlock) void render_information_shape_kernel(
    const float* __restrict__ depth, const float* __restrict__ target, const float* __restrict__ sdf, int R,
    long long sdf_view_stride, const float* __restrict__ jac, int Tp, int T, long long jac_view_stride,
    const float* __restrict__ pos, const float* __restrict__ quat, const float* __restrict__ inv_scale, int W, int H,
    float cx, float cy, float fx, float fy, float rfx, float rfy, float inlier_threshold, unsigned* __restrict__ flags,
    float* __restrict__ records) {
  __shared__ ShapeLds lds;
  using PB = Patch<kPatchWBwd>;
  const int b = blockIdx.z;
  const size_t tile = ((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int px0 = blockIdx.x * kInfoTileW, py0 = blockIdx.y * kInfoTileH;
  const int F = 10 + T;
  ViewSetup s;
  info_pose(b, pos, quat, inv_scale, s);
  if (info_tile_culled(s, px0, py0, cx, cy, fx, fy)) {   // workgroup-uniform
    if (tid == 0) flags[tile] = 0u;
    return;
  }
  const float* zimg = depth + (size_t)b * H * W;
  const float* timg = target + (size_t)b * H * W;

  // the tile's pixels and the inclusion rule: render_information_kernel's statements
  float zs[kInfoSubs], ts[kInfoSubs];
  bool inc[kInfoSubs], any = false;
  const int row = py0 + PB::oy(wave) + PB::y(lane);
#pragma unroll
  for (int sub = 0; sub < kInfoSubs; ++sub) {
    const int col = px0 + sub * kSubW + PB::ox(wave) + PB::x(lane);
    zs[sub] = (col < W && row < H) ? zimg[(size_t)row * W + col] : 0.0f;
  }
#pragma unroll
  for (int sub = 0; sub < kInfoSubs; ++sub) {
    const int col = px0 + sub * kSubW + PB::ox(wave) + PB::x(lane);
    const float z = zs[sub];
    const float t = z > 0.0f ? timg[(size_t)row * W + col] : 0.0f;
    ts[sub] = t;
    inc[sub] = z > 0.0f && t > 0.0f && (inlier_threshold == 0.0f || __fdiv_rn(fabsf(t - z), t) < inlier_threshold);
    any = any || inc[sub];
  }
  if (!__syncthreads_or(any)) {   // workgroup-uniform
    if (tid == 0) flags[tile] = 0u;
    return;
  }

  const float* vol = sdf + (size_t)b * sdf_view_stride;
  const float* jv = jac + (size_t)b * jac_view_stride;
  float* blk = lds.feat[wave];
  f32x16 acc;
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0f;
#pragma unroll
  for (int sub = 0; sub < kInfoSubs; ++sub) {
    if (__ballot(inc[sub]) == 0ull) continue;   // wave-uniform: no gathers, no products
    float f[kShapeF];
#pragma unroll
    for (int k = 0; k < kShapeF; ++k) f[k] = 0.0f;
    if (inc[sub]) {
      const int col = px0 + sub * kSubW + PB::ox(wave) + PB::x(lane);
      float dd[8];
      pixel_derivatives<RT>(s, vol, R, row, col, zs[sub], cx, cy, rfx, rfy, dd);
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = dd[k];
      latent_features<RT>(s, jv, Tp, T, R, row, col, zs[sub], cx, cy, rfx, rfy, f);
      const float r = zs[sub] - ts[sub];
#pragma unroll
      for (int k = 9; k < kShapeF; ++k) f[k] = k == 8 + T ? r : k == 9 + T ? 1.0f : f[k];
    }
    f32x4* mine = reinterpret_cast<f32x4*>(blk + lane * kShapeF);
#pragma unroll
    for (int k = 0; k < kShapeF / 4; ++k) mine[k] = f32x4{f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]};
    // the wave's own rows, read back across lanes (as information.hip: the LDS serves a wave's accesses in order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll 8
    for (int g = 0; g < 32; ++g) {
      const float x = blk[64 * g + lane];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x, x, acc, 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  // C/D layout: column = lane & 31, row = (register & 3) + 8 (register >> 2) + 4 (lane >> 5); into the wave's own block
#pragma unroll
  for (int k = 0; k < 16; ++k) blk[((k & 3) + 8 * (k >> 2) + 4 * (lane >> 5)) * 32 + (lane & 31)] = acc[k];
  __syncthreads();
  for (int e = tid; e < F * F; e += kInfoBlock) {
    const int w = (e / F) * 32 + e % F;
    records[tile * (size_t)(F * F) + e] = (lds.feat[0][w] + lds.feat[1][w]) + (lds.feat[2][w] + lds.feat[3][w]);
  }
  if (tid == 0) flags[tile] = 1u;
}

// Fixed-order sum of a view's tile records in double: information_reduce_kernel's order (chunk c sums its share of the
// tiles in tile order, a tile without a record adds +0, then the chunks in chunk order), 128 entries of the record per
// pass.  grid: B; kShapeChunks x kShapeLanes threads.
__global__ __launch_bounds__(kShapeChunks * kShapeLanes) void information_shape_reduce_kernel(
    const unsigned* __restrict__ flags, const float* __restrict__ records, int tiles, int rec, double* __restrict__ gram) {
  __shared__ double part[kShapeChunks][kShapeLanes];
  const int b = blockIdx.x, lane = threadIdx.x % kShapeLanes, c = threadIdx.x / kShapeLanes;
  const unsigned* fl = flags + (size_t)b * tiles;
  const float* recs = records + (size_t)b * tiles * rec;
  const int per = (tiles + kShapeChunks - 1) / kShapeChunks;
  const int t0 = c * per, t1 = min(t0 + per, tiles);
  for (int e0 = 0; e0 < rec; e0 += kShapeLanes) {   // block-uniform
    const int e = e0 + lane;
    double a = 0.0;
    if (e < rec) {
      for (int t = t0; t < t1; t += 8) {
        unsigned f[8];
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (t + j < t1) ? fl[t + j] : 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = f[j] != 0u ? recs[(size_t)(t + j) * rec + e] : 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a += (double)v[j];
      }
    }
    part[c][lane] = a;
    __syncthreads();
    if (c == 0 && e < rec) {
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < kShapeChunks; ++k) sum += part[k][lane];
      gram[(size_t)b * rec + e] = sum;
    }
    __syncthreads();
  }
}

inline size_t shape_record_floats(int T) { return (size_t)(10 + T) * (10 + T); }

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_render_information_shape_workspace_bytes(int B, int W, int H, int T) {
  if (!info_sizes_ok(B, W, H) || T < 1 || T > kShapeMaxT) return 0;
  return info_flag_bytes(B, W, H) + (size_t)B * info_tiles_x(W) * info_tiles_y(H) * shape_record_floats(T) * sizeof(float);
}

extern "C" int sdfr_render_information_shape(const float* depth, const float* target, const float* sdf, int R,
                                             long long sdf_view_stride, const float* jac, int Tp, int T,
                                             long long jac_view_stride, const float* pos, const float* quat,
                                             const float* inv_scale, int B, int W, int H, float cx, float cy, float fx,
                                             float fy, float inlier_threshold, double* gram, void* workspace,
                                             size_t workspace_bytes, int device, void* stream) {
  const char* fn = "sdfr_render_information_shape";
  if (B < 1 || W < 1 || H < 1) return fail(SDFR_E_INVALID, "%s: B=%d, W=%d, H=%d must be >= 1", fn, B, W, H);
  if (R < 2 || R > 1023) return fail(SDFR_E_INVALID, "%s: R=%d out of range [2,1023]", fn, R);
  if (T < 1 || T > kShapeMaxT) return fail(SDFR_E_INVALID, "%s: T=%d out of range [1,%d]", fn, T, kShapeMaxT);
  if (Tp < T || (Tp & 3)) return fail(SDFR_E_INVALID, "%s: Tp=%d must be a multiple of 4 and at least T=%d", fn, Tp, T);
  if (!info_sizes_ok(B, W, H)) return fail(SDFR_E_INVALID, "%s: B=%d views of %d x %d pixels are too many", fn, B, W, H);
  if (!(fx != 0.0f) || !(fy != 0.0f)) return fail(SDFR_E_INVALID, "%s: focal length must be non-zero", fn);
  if (!(inlier_threshold >= 0.0f) || !(inlier_threshold < INFINITY))
    return fail(SDFR_E_INVALID, "%s: inlier_threshold=%g must be >= 0 and finite", fn, (double)inlier_threshold);
  if (sdf_view_stride != 0 && sdf_view_stride < (long long)R * R * R)
    return fail(SDFR_E_INVALID, "%s: sdf_view_stride must be 0 or >= R^3", fn);
  if (jac_view_stride != 0 && jac_view_stride < (long long)R * R * R * Tp)
    return fail(SDFR_E_INVALID, "%s: jac_view_stride must be 0 or >= R^3 Tp", fn);
  if (!depth || !target || !sdf || !jac || !pos || !quat || !inv_scale || !gram || !workspace)
    return fail(SDFR_E_INVALID, "%s: NULL pointer argument", fn);
  const size_t need = sdfr_render_information_shape_workspace_bytes(B, W, H, T);
  if (workspace_bytes < need)
    return fail(SDFR_E_INVALID, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
  if (((uintptr_t)workspace & 127u) || ((uintptr_t)gram & 7u) || ((uintptr_t)jac & 15u) || (jac_view_stride & 3))
    return fail(SDFR_E_INVALID, "%s: workspace must be 128-byte, jac (and its view stride) 16-byte and gram 8-byte aligned", fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int ntx = info_tiles_x(W), nty = info_tiles_y(H);
  unsigned* flags = (unsigned*)workspace;
  float* records = (float*)((char*)workspace + info_flag_bytes(B, W, H));
  const float rfx = (float)(1.0 / (double)fx), rfy = (float)(1.0 / (double)fy);
  const dim3 grid((unsigned)ntx, (unsigned)nty, (unsigned)B);
  if (R == 64)
    hipLaunchKernelGGL((render_information_shape_kernel<64>), grid, dim3(kInfoBlock), 0, st, depth, target, sdf, R,
                       sdf_view_stride, jac, Tp, T, jac_view_stride, pos, quat, inv_scale, W, H, cx, cy, fx, fy, rfx, rfy,
                       inlier_threshold, flags, records);
  else
    hipLaunchKernelGGL((render_information_shape_kernel<0>), grid, dim3(kInfoBlock), 0, st, depth, target, sdf, R,
                       sdf_view_stride, jac, Tp, T, jac_view_stride, pos, quat, inv_scale, W, H, cx, cy, fx, fy, rfx, rfy,
                       inlier_threshold, flags, records);
  hipLaunchKernelGGL(information_shape_reduce_kernel, dim3((unsigned)B), dim3(kShapeChunks * kShapeLanes), 0, st, flags,
                     records, ntx * nty, (int)shape_record_floats(T), gram);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
