// information.hip -- Gauss-Newton information of the depth residual (gfx950 only): sdfr_render_information.
//
// Per view, the 10 x 10 Gram matrix of the per-pixel feature vector f = (d0 .. d7, r, 1) over the included pixels:
// d = d depth / d (px, py, pz, qx, qy, qz, qw, inv_scale) -- the per-pixel vector the backward multiplies by its
// upstream gradient and sums away (render.hip, backward_tile: the same hit point, cell, trilinear gradient and terms,
// with upstream gradient 1) --, r = depth - target.  [:8,:8] is J^T J, [:8,8] J^T r, [8,8] sum r^2, [9,9] the count.
//
// A Gram matrix is the GEMM F^T F with K = pixels.  For v_mfma_f32_16x16x4_f32 lane l holds A[l & 15][l >> 4] and
// B[l >> 4][l & 15]: with A = F^T and B = F both operands are the SAME register, feature l & 15 of pixel 4 g + (l >> 4)
// of k-step g.  A lane writes its pixel's features as a row of 16 floats into its wave's 4 KiB LDS block and reads word
// 64 g + l back: sixteen MFMAs per 64 pixels leave the 16 x 16 block in four accumulator registers.  The instruction is
// a k-ordered fma chain with one rounding per product, so the sums have ONE order -- the same bits on every run -- and
// entry (i, j) and entry (j, i) see the same products in the same order: the matrix is symmetric bit for bit.  An
// excluded pixel's row is all zeros (never a product with a possibly non-finite derivative), an included pixel's last
// feature is 1: entry (9, 9) is the count, exact in fp32 far beyond a tile's 512 pixels.
//
// Two launches: the tile kernel over all views (a tile without an included pixel writes a 0 flag and nothing else),
// then a fixed-order sum of each view's tile records in double.  The tiling is a function of (W, H) alone, so a view's
// matrix does not depend on which other views share the call.
#include <climits>
#include <cmath>

#include "information_device.hpp"

namespace sdfr {
namespace {

constexpr int kInfoN = 10;                              // features per pixel
constexpr int kInfoRec = kInfoN * kInfoN;               // floats of a tile record
constexpr int kInfoChunks = 8;                          // the reduce kernel: chunks of a view's tiles summed side by side
constexpr int kInfoLanes = 128;                         // ... by this many threads each (kInfoRec of them at work)
static_assert(kInfoRec <= kInfoLanes, "one thread per entry");

typedef float f32x4 __attribute__((ext_vector_type(4)));

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
  using PB = Patch<kPatchWBwd>;
  const int b = blockIdx.z;
  const size_t tile = ((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int px0 = blockIdx.x * kInfoTileW, py0 = blockIdx.y * kInfoTileH;
  // the view's pose first (scalar loads): three tiles out of four lie outside the object and leave without a pixel read
  ViewSetup s;
  info_pose(b, pos, quat, inv_scale, s);
  if (info_tile_culled(s, px0, py0, cx, cy, fx, fy)) {   // workgroup-uniform
    if (tid == 0) flags[tile] = 0u;
    return;
  }
  const float* zimg = depth + (size_t)b * H * W;
  const float* timg = target + (size_t)b * H * W;

  // the tile's pixels: estimate, then the target of the hit pixels only; the inclusion rule
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
    // overlap, and the relative inlier rule with an IEEE subtraction and DIVISION: numpy float32 gives the same set
    inc[sub] = z > 0.0f && t > 0.0f && (inlier_threshold == 0.0f || __fdiv_rn(fabsf(t - z), t) < inlier_threshold);
    any = any || inc[sub];
  }
  if (!__syncthreads_or(any)) {   // workgroup-uniform
    if (tid == 0) flags[tile] = 0u;
    return;
  }

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
    // the wave's own rows, read back across lanes: the LDS serves a wave's accesses in order; the fences keep the
    // compiler from moving them and wait for the writes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
    for (int g = 0; g < 16; g += 2) {
      const float x0 = blk[64 * g + lane], x1 = blk[64 * (g + 1) + lane];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, x0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, x1, acc1, 0, 0, 0);
    }
    // (the next sub-tile's rows go into the same block: behind these reads)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
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

// Fixed-order sum of a view's tile records in double.  grid: B; kInfoChunks x kInfoLanes threads: chunk c sums its
// share of the tiles in tile order (a tile without a record adds +0), then the chunks are added in chunk order.
__global__ __launch_bounds__(kInfoChunks * kInfoLanes) void information_reduce_kernel(
    const unsigned* __restrict__ flags, const float* __restrict__ records, int tiles, double* __restrict__ gram) {
  __shared__ double part[kInfoChunks][kInfoRec];
  const int b = blockIdx.x, e = threadIdx.x % kInfoLanes, c = threadIdx.x / kInfoLanes;
  const unsigned* fl = flags + (size_t)b * tiles;
  const float* rec = records + (size_t)b * tiles * kInfoRec;
  const int per = (tiles + kInfoChunks - 1) / kInfoChunks;
  const int t0 = c * per, t1 = min(t0 + per, tiles);
  if (e < kInfoRec) {
    // eight tiles per round: the next round's flags are on their way while this round's records are (a flag and the
    // record behind it are two dependent round trips otherwise); a tile past the chunk's end counts as one without a record
    double a = 0.0;
    unsigned f[8], fn[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (t0 + j < t1) ? fl[t0 + j] : 0u;
    for (int t = t0; t < t1; t += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) fn[j] = (t + 8 + j < t1) ? fl[t + 8 + j] : 0u;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = f[j] != 0u ? rec[(size_t)(t + j) * kInfoRec + e] : 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) a += (double)v[j];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = fn[j];
    }
    part[c][e] = a;
  }
  __syncthreads();
  if (threadIdx.x < kInfoRec) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < kInfoChunks; ++k) a += part[k][threadIdx.x];
    gram[(size_t)b * kInfoRec + threadIdx.x] = a;
  }
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_render_information_workspace_bytes(int B, int W, int H) {
  if (!info_sizes_ok(B, W, H)) return 0;
  return info_flag_bytes(B, W, H) + (size_t)B * info_tiles_x(W) * info_tiles_y(H) * kInfoRec * sizeof(float);
}

extern "C" int sdfr_render_information(const float* depth, const float* target, const float* sdf, int R,
                                       long long sdf_view_stride, const float* pos, const float* quat,
                                       const float* inv_scale, int B, int W, int H, float cx, float cy, float fx,
                                       float fy, float inlier_threshold, double* gram, void* workspace,
                                       size_t workspace_bytes, int device, void* stream) {
  const char* fn = "sdfr_render_information";
  if (B < 1 || W < 1 || H < 1) return fail(SDFR_E_INVALID, "%s: B=%d, W=%d, H=%d must be >= 1", fn, B, W, H);
  if (R < 2 || R > 1023) return fail(SDFR_E_INVALID, "%s: R=%d out of range [2,1023]", fn, R);
  if (!info_sizes_ok(B, W, H)) return fail(SDFR_E_INVALID, "%s: B=%d views of %d x %d pixels are too many", fn, B, W, H);
  if (!(fx != 0.0f) || !(fy != 0.0f)) return fail(SDFR_E_INVALID, "%s: focal length must be non-zero", fn);
  if (!(inlier_threshold >= 0.0f) || !(inlier_threshold < INFINITY))
    return fail(SDFR_E_INVALID, "%s: inlier_threshold=%g must be >= 0 and finite", fn, (double)inlier_threshold);
  if (sdf_view_stride != 0 && sdf_view_stride < (long long)R * R * R)
    return fail(SDFR_E_INVALID, "%s: sdf_view_stride must be 0 or >= R^3", fn);
  if (!depth || !target || !sdf || !pos || !quat || !inv_scale || !gram || !workspace)
    return fail(SDFR_E_INVALID, "%s: NULL pointer argument", fn);
  const size_t need = sdfr_render_information_workspace_bytes(B, W, H);
  if (workspace_bytes < need)
    return fail(SDFR_E_INVALID, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
  if (((uintptr_t)workspace & 127u) || ((uintptr_t)gram & 7u))
    return fail(SDFR_E_INVALID, "%s: workspace must be 128-byte and gram 8-byte aligned", fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int ntx = info_tiles_x(W), nty = info_tiles_y(H);
  unsigned* flags = (unsigned*)workspace;
  float* records = (float*)((char*)workspace + info_flag_bytes(B, W, H));
  const float rfx = (float)(1.0 / (double)fx), rfy = (float)(1.0 / (double)fy);
  const dim3 grid((unsigned)ntx, (unsigned)nty, (unsigned)B);
  if (R == 64)
    hipLaunchKernelGGL((render_information_kernel<64>), grid, dim3(kInfoBlock), 0, st, depth, target, sdf, R,
                       sdf_view_stride, pos, quat, inv_scale, W, H, cx, cy, fx, fy, rfx, rfy, inlier_threshold, flags,
                       records);
  else
    hipLaunchKernelGGL((render_information_kernel<0>), grid, dim3(kInfoBlock), 0, st, depth, target, sdf, R,
                       sdf_view_stride, pos, quat, inv_scale, W, H, cx, cy, fx, fy, rfx, rfy, inlier_threshold, flags,
                       records);
  hipLaunchKernelGGL(information_reduce_kernel, dim3((unsigned)B), dim3(kInfoChunks * kInfoLanes), 0, st, flags,
                     records, ntx * nty, gram);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
