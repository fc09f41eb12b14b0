// information.hip -- Gauss-Newton information of the depth residual (gfx950 only): sdfr_render_information (the pose)
// and sdfr_render_information_shape (pose AND latent).
//
// Pose.  Per view, the 10 x 10 Gram matrix of the per-pixel feature vector f = (d0 .. d7, r, 1) over the included pixels:
// d = d depth / d (px, py, pz, qx, qy, qz, qw, inv_scale) -- the per-pixel vector the backward multiplies by its
// upstream gradient and sums away (render.hip, backward_tile: the same hit point, cell, trilinear gradient and terms,
// with upstream gradient 1) --, r = depth - target.  [:8,:8] is J^T J, [:8,8] J^T r, [8,8] sum r^2, [9,9] the count.
//
// Pose and latent.  The F x F matrix, F = 10 + T, of f = (d0 .. d7, s0 .. s_{T-1}, r, 1) over the same pixels: one
// prologue (information_device.hpp: tile cull, inclusion rule) and one pixel_derivatives serve both kernels.
// s_t = d depth / d z_t: the backward's d depth / d SDF weights of a hit pixel are f * (the trilinear weights of its
// cell), f = scale |d.z| (render.hip, backward_tile, the SDFR_SDF_GRAD_EXACT branch), so s_t = f * trilerp(jac[.][t]) at
// the pixel's cell with the pixel's offsets -- eight more gathers of Tp floats at the cell info_latent_cell names
// (latent_features, information_gram.hpp).
//
// The Gram products.  The joint kernel's is the 32-wide one of information_gram.hpp.  The pose-only kernel has its own,
// on purpose -- another instruction, another summation order, half the LDS: for v_mfma_f32_16x16x4_f32 lane l holds
// A[l & 15][l >> 4] and B[l >> 4][l & 15]: with A = F^T and B = F both operands are the SAME register, feature l & 15 of
// pixel 4 g + (l >> 4) of k-step g.  A lane writes its pixel's features as a row of 16 floats into its wave's 4 KiB LDS
// block and reads word 64 g + l back: sixteen MFMAs per 64 pixels leave the 16 x 16 block in four accumulator registers.
// As there, a k-ordered fma chain: one order, symmetric bit for bit, an excluded pixel's row all zeros, entry (9, 9) the
// count, exact in fp32 far beyond a tile's 512 pixels.
//
// Two launches either way: the tile kernel over all views (a tile without an included pixel writes a 0 flag and nothing
// else), then a fixed-order sum of each view's tile records in double.  The tiling is a function of (W, H) alone, so a
// view's matrix does not depend on which other views share the call.
#include <climits>
#include <cmath>

#include "information_device.hpp"
#include "information_gram.hpp"

namespace sdfr {
namespace {

constexpr int kInfoN = 10;                              // features per pixel, pose only
constexpr int kInfoRec = kInfoN * kInfoN;               // floats of its tile record
constexpr int kInfoChunks = 8;                          // the reduce kernel: chunks of a view's tiles summed side by side
constexpr int kInfoLanes = 128;                         // ... by this many threads each, 128 entries of the record per pass
static_assert(kInfoBlock == 64 * kGramWaves, "one Gram block per wave");

struct InfoLds {
  float feat[kInfoBlock / 64][64 * 16];   // per wave: [pixel][feature], features 10 .. 15 are zero padding
  float wave_acc[kInfoBlock / 64][256];   // per wave: its 16 x 16 block, row-major
};

// grid: (tiles in x, tiles in y, B).  flags [B][tiles]: 1 = the tile has a record; records [B][tiles][kInfoRec].
template <int RT>
__global__ __launch_bounds__(kInfoBlock) void render_information_kernel(
    const float* __restrict__ depth, const float* __restrict__ target, const float* __restrict__ sdf, int R,
    long long sdf_view_stride, const float* __restrict__ pos, const float* __restrict__ quat,
    const float* __restrict__ inv_scale, int W, int H, float cx, float cy, float fx, float fy, float rfx, float rfy,
    float inlier_threshold, unsigned* __restrict__ flags, float* __restrict__ records) {
  __shared__ InfoLds lds;
  const int b = blockIdx.z;
  const size_t tile = ((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  using PB = Patch<kPatchWBwd>;
  const int px0 = blockIdx.x * kInfoTileW;
  ViewSetup s;
  int row;
  float zs[kInfoSubs], ts[kInfoSubs];
  bool inc[kInfoSubs];
  if (!info_tile_begin(depth, target, pos, quat, inv_scale, W, H, cx, cy, fx, fy, inlier_threshold, flags + tile, s, row, zs,
                       ts, inc))
    return;

  const float* vol = sdf + (size_t)b * sdf_view_stride;
  float* blk = lds.feat[wave];
  f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int sub = 0; sub < kInfoSubs; ++sub) {
    if (__ballot(inc[sub]) == 0ull) continue;   // wave-uniform: no gathers, no products
    float f[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (inc[sub]) {
      const int col = px0 + sub * kSubW + PB::ox(wave) + PB::x(lane);
      float dd[8];
      pixel_derivatives<RT>(s, vol, R, row, col, zs[sub], cx, cy, rfx, rfy, dd);
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = dd[k];
      f[8] = zs[sub] - ts[sub];
      f[9] = 1.0f;
    }
    f32x4* mine = reinterpret_cast<f32x4*>(blk + lane * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) mine[k] = f32x4{f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]};
    gram_wave_sync();   // the wave's own rows, read back across lanes
#pragma unroll
    for (int g = 0; g < 16; g += 2) {
      const float x0 = blk[64 * g + lane], x1 = blk[64 * (g + 1) + lane];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, x0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, x1, acc1, 0, 0, 0);
    }
    gram_wave_sync();   // (the next sub-tile's rows go into the same block: behind these reads)
  }
  // C/D layout: column = lane & 15, row = 4 (lane >> 4) + register
  const f32x4 acc = acc0 + acc1;
#pragma unroll
  for (int k = 0; k < 4; ++k) lds.wave_acc[wave][(4 * (lane >> 4) + k) * 16 + (lane & 15)] = acc[k];
  __syncthreads();
  if (tid < kInfoRec) {
    const int e = (tid / kInfoN) * 16 + tid % kInfoN;
    records[tile * kInfoRec + tid] =
        (lds.wave_acc[0][e] + lds.wave_acc[1][e]) + (lds.wave_acc[2][e] + lds.wave_acc[3][e]);
  }
  if (tid == 0) flags[tile] = 1u;
}

// grid: (tiles in x, tiles in y, B).  flags [B][tiles]: 1 = the tile has a record; records [B][tiles][F F], F = 10 + T.
template <int RT>
__global__ __launch_bounds__(kInfoBlock) void render_information_shape_kernel(
    const float* __restrict__ depth, const float* __restrict__ target, const float* __restrict__ sdf, int R,
    long long sdf_view_stride, const float* __restrict__ jac, int Tp, int T, long long jac_view_stride,
    const float* __restrict__ pos, const float* __restrict__ quat, const float* __restrict__ inv_scale, int W, int H,
    float cx, float cy, float fx, float fy, float rfx, float rfy, float inlier_threshold, unsigned* __restrict__ flags,
    float* __restrict__ records) {
  __shared__ GramBlock lds[kGramWaves];
  const int b = blockIdx.z;
  const size_t tile = ((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int Rr = RT > 0 ? RT : R;
  const int F = 10 + T;
  using PB = Patch<kPatchWBwd>;
  const int px0 = blockIdx.x * kInfoTileW;
  ViewSetup s;
  int row;
  float zs[kInfoSubs], ts[kInfoSubs];
  bool inc[kInfoSubs];
  if (!info_tile_begin(depth, target, pos, quat, inv_scale, W, H, cx, cy, fx, fy, inlier_threshold, flags + tile, s, row, zs,
                       ts, inc))
    return;

  const float* vol = sdf + (size_t)b * sdf_view_stride;
  const float* jv = jac + (size_t)b * jac_view_stride;
  f32x16 acc;
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0f;
#pragma unroll
  for (int sub = 0; sub < kInfoSubs; ++sub) {
    if (__ballot(inc[sub]) == 0ull) continue;   // wave-uniform: no gathers, no products
    float f[kGramF];
#pragma unroll
    for (int k = 0; k < kGramF; ++k) f[k] = 0.0f;
    if (inc[sub]) {
      const int col = px0 + sub * kSubW + PB::ox(wave) + PB::x(lane);
      float dd[8], weight;
      Cell c;
      pixel_derivatives<RT>(s, vol, R, row, col, zs[sub], cx, cy, rfx, rfy, dd);
      info_latent_cell<RT>(s, R, row, col, zs[sub], cx, cy, rfx, rfy, c, weight);
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = dd[k];
      latent_features(c, jv, Tp, T, Rr, weight, f);
      const float r = zs[sub] - ts[sub];
#pragma unroll
      for (int k = 9; k < kGramF; ++k) f[k] = k == 8 + T ? r : k == 9 + T ? 1.0f : f[k];
    }
    gram32_accumulate(f, lds[wave], lane, acc);
  }
  gram32_store(acc, lds[wave], lane);
  __syncthreads();
  gram32_record(lds, F, tid, records + tile * (size_t)(F * F));
  if (tid == 0) flags[tile] = 1u;
}

// Fixed-order sum of a view's tile records of `rec` floats in double.  grid: B; kInfoChunks x kInfoLanes threads: chunk c
// sums its share of the tiles in tile order (a tile without a record adds +0), then the chunks are added in chunk order;
// kInfoLanes entries of the record per pass.  REC > 0: the record length at compile time (the pose-only record: one
// pass, constant strides -- a single view's reduce is a chain of dependent round trips and an LM iteration waits for it).
template <int REC>
__global__ __launch_bounds__(kInfoChunks * kInfoLanes) void information_reduce_kernel(
    const unsigned* __restrict__ flags, const float* __restrict__ records, int tiles, int rec_arg,
    double* __restrict__ gram) {
  constexpr int kWidth = REC > 0 && REC < kInfoLanes ? REC : kInfoLanes;
  __shared__ double part[kInfoChunks][kWidth];
  const int rec = REC > 0 ? REC : rec_arg;
  const int b = blockIdx.x, lane = threadIdx.x % kInfoLanes, c = threadIdx.x / kInfoLanes;
  const unsigned* fl = flags + (size_t)b * tiles;
  const float* recs = records + (size_t)b * tiles * rec;
  const int per = (tiles + kInfoChunks - 1) / kInfoChunks;
  const int t0 = c * per, t1 = min(t0 + per, tiles);
  for (int e0 = 0; e0 < rec; e0 += kInfoLanes) {   // block-uniform
    const int e = e0 + lane;
    double a = 0.0;
    if (e < rec) {
      // eight tiles per round: the next round's flags are on their way while this round's records are (a flag and the
      // record behind it are two dependent round trips otherwise); a tile past the chunk's end counts as one without a record
      unsigned f[8], fn[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = (t0 + j < t1) ? fl[t0 + j] : 0u;
      for (int t = t0; t < t1; t += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) fn[j] = (t + 8 + j < t1) ? fl[t + 8 + j] : 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = f[j] != 0u ? recs[(size_t)(t + j) * rec + e] : 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a += (double)v[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = fn[j];
      }
    }
    if (lane < kWidth) part[c][lane] = a;
    __syncthreads();
    if (c == 0 && e < rec) {
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < kInfoChunks; ++k) sum += part[k][lane];
      gram[(size_t)b * rec + e] = sum;
    }
    __syncthreads();
  }
}

inline size_t info_workspace_bytes(int B, int W, int H, size_t rec) {
  return info_flag_bytes(B, W, H) + (size_t)B * info_tiles_x(W) * info_tiles_y(H) * rec * sizeof(float);
}

// the Jacobian arguments of the joint entry
struct InfoJac {
  const float* jac;
  int Tp, T;
  long long view_stride;
};

// The argument checks of the two depth entries, in one order; j = nullptr: the pose-only entry.  `null_arg`: one of the
// entry's pointers is NULL; `need`: its _workspace_bytes.
int info_check_args(const char* fn, int B, int W, int H, int R, float fx, float fy, float inlier_threshold,
                    long long sdf_view_stride, const InfoJac* j, bool null_arg, const void* workspace,
                    size_t workspace_bytes, size_t need, const double* gram) {
  if (B < 1 || W < 1 || H < 1) return fail(SDFR_E_INVALID, "%s: B=%d, W=%d, H=%d must be >= 1", fn, B, W, H);
  if (R < 2 || R > 1023) return fail(SDFR_E_INVALID, "%s: R=%d out of range [2,1023]", fn, R);
  if (j && (j->T < 1 || j->T > SDFR_INFO_MAX_TANGENTS))
    return fail(SDFR_E_INVALID, "%s: T=%d out of range [1,%d]", fn, j->T, SDFR_INFO_MAX_TANGENTS);
  if (j && (j->Tp < j->T || (j->Tp & 3)))
    return fail(SDFR_E_INVALID, "%s: Tp=%d must be a multiple of 4 and at least T=%d", fn, j->Tp, j->T);
  if (!info_sizes_ok(B, W, H)) return fail(SDFR_E_INVALID, "%s: B=%d views of %d x %d pixels are too many", fn, B, W, H);
  if (!(fx != 0.0f) || !(fy != 0.0f)) return fail(SDFR_E_INVALID, "%s: focal length must be non-zero", fn);
  if (!(inlier_threshold >= 0.0f) || !(inlier_threshold < INFINITY))
    return fail(SDFR_E_INVALID, "%s: inlier_threshold=%g must be >= 0 and finite", fn, (double)inlier_threshold);
  if (sdf_view_stride != 0 && sdf_view_stride < (long long)R * R * R)
    return fail(SDFR_E_INVALID, "%s: sdf_view_stride must be 0 or >= R^3", fn);
  if (j && j->view_stride != 0 && j->view_stride < (long long)R * R * R * j->Tp)
    return fail(SDFR_E_INVALID, "%s: jac_view_stride must be 0 or >= R^3 Tp", fn);
  if (null_arg || !gram || !workspace) return fail(SDFR_E_INVALID, "%s: NULL pointer argument", fn);
  if (workspace_bytes < need)
    return fail(SDFR_E_INVALID, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
  const bool ws_gram = ((uintptr_t)workspace & 127u) || ((uintptr_t)gram & 7u);
  if (!j && ws_gram) return fail(SDFR_E_INVALID, "%s: workspace must be 128-byte and gram 8-byte aligned", fn);
  if (j && (ws_gram || ((uintptr_t)j->jac & 15u) || (j->view_stride & 3)))
    return fail(SDFR_E_INVALID, "%s: workspace must be 128-byte, jac (and its view stride) 16-byte and gram 8-byte aligned", fn);
  return 0;
}

// a call's launch geometry and its workspace carved into flags [B][tiles] and records [B][tiles][rec]
struct InfoLaunch {
  dim3 grid;
  int tiles;
  unsigned* flags;
  float* records;
  float rfx, rfy;
};
InfoLaunch info_launch(void* workspace, int B, int W, int H, float fx, float fy) {
  const int ntx = info_tiles_x(W), nty = info_tiles_y(H);
  return {dim3((unsigned)ntx, (unsigned)nty, (unsigned)B), ntx * nty, (unsigned*)workspace,
          (float*)((char*)workspace + info_flag_bytes(B, W, H)), (float)(1.0 / (double)fx), (float)(1.0 / (double)fy)};
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_render_information_workspace_bytes(int B, int W, int H) {
  if (!info_sizes_ok(B, W, H)) return 0;
  return info_workspace_bytes(B, W, H, kInfoRec);
}

extern "C" int sdfr_render_information(const float* depth, const float* target, const float* sdf, int R,
                                       long long sdf_view_stride, const float* pos, const float* quat,
                                       const float* inv_scale, int B, int W, int H, float cx, float cy, float fx,
                                       float fy, float inlier_threshold, double* gram, void* workspace,
                                       size_t workspace_bytes, int device, void* stream) {
  if (const int rc = info_check_args("sdfr_render_information", B, W, H, R, fx, fy, inlier_threshold, sdf_view_stride,
                                     nullptr, !depth || !target || !sdf || !pos || !quat || !inv_scale, workspace,
                                     workspace_bytes, sdfr_render_information_workspace_bytes(B, W, H), gram))
    return rc;
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const InfoLaunch l = info_launch(workspace, B, W, H, fx, fy);
  if (R == 64)
    hipLaunchKernelGGL((render_information_kernel<64>), l.grid, dim3(kInfoBlock), 0, st, depth, target, sdf, R,
                       sdf_view_stride, pos, quat, inv_scale, W, H, cx, cy, fx, fy, l.rfx, l.rfy, inlier_threshold,
                       l.flags, l.records);
  else
    hipLaunchKernelGGL((render_information_kernel<0>), l.grid, dim3(kInfoBlock), 0, st, depth, target, sdf, R,
                       sdf_view_stride, pos, quat, inv_scale, W, H, cx, cy, fx, fy, l.rfx, l.rfy, inlier_threshold,
                       l.flags, l.records);
  hipLaunchKernelGGL(information_reduce_kernel<kInfoRec>, dim3((unsigned)B), dim3(kInfoChunks * kInfoLanes), 0, st,
                     l.flags, l.records, l.tiles, kInfoRec, gram);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" size_t sdfr_render_information_shape_workspace_bytes(int B, int W, int H, int T) {
  if (!info_sizes_ok(B, W, H) || T < 1 || T > SDFR_INFO_MAX_TANGENTS) return 0;
  return info_workspace_bytes(B, W, H, (size_t)(10 + T) * (10 + T));
}

extern "C" int sdfr_render_information_shape(const float* depth, const float* target, const float* sdf, int R,
                                             long long sdf_view_stride, const float* jac, int Tp, int T,
                                             long long jac_view_stride, const float* pos, const float* quat,
                                             const float* inv_scale, int B, int W, int H, float cx, float cy, float fx,
                                             float fy, float inlier_threshold, double* gram, void* workspace,
                                             size_t workspace_bytes, int device, void* stream) {
  const InfoJac j{jac, Tp, T, jac_view_stride};
  if (const int rc = info_check_args("sdfr_render_information_shape", B, W, H, R, fx, fy, inlier_threshold,
                                     sdf_view_stride, &j, !depth || !target || !sdf || !jac || !pos || !quat || !inv_scale,
                                     workspace, workspace_bytes,
                                     sdfr_render_information_shape_workspace_bytes(B, W, H, T), gram))
    return rc;
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const InfoLaunch l = info_launch(workspace, B, W, H, fx, fy);
  if (R == 64)
    hipLaunchKernelGGL((render_information_shape_kernel<64>), l.grid, dim3(kInfoBlock), 0, st, depth, target, sdf, R,
                       sdf_view_stride, jac, Tp, T, jac_view_stride, pos, quat, inv_scale, W, H, cx, cy, fx, fy, l.rfx,
                       l.rfy, inlier_threshold, l.flags, l.records);
  else
    hipLaunchKernelGGL((render_information_shape_kernel<0>), l.grid, dim3(kInfoBlock), 0, st, depth, target, sdf, R,
                       sdf_view_stride, jac, Tp, T, jac_view_stride, pos, quat, inv_scale, W, H, cx, cy, fx, fy, l.rfx,
                       l.rfy, inlier_threshold, l.flags, l.records);
  hipLaunchKernelGGL(information_reduce_kernel<0>, dim3((unsigned)B), dim3(kInfoChunks * kInfoLanes), 0, st, l.flags,
                     l.records, l.tiles, (10 + T) * (10 + T), gram);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
