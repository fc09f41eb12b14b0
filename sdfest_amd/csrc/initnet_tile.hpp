// initnet_tile.hpp -- the per-point layer of the initialisation network for ONE tile of 64 rows x 64 columns of one
// point set: staging, the fp32 MFMA loop over the k chunks, and the epilogue (bias, folded BatchNorm, ReLU, residual,
// column maximum).  pointnet_layer_kernel (initnet.hip: one set per launch, row tiles in a grid-stride loop) and
// pointnet_layer_batch_kernel (initnet_eval.hip: N sets per launch, one tile per workgroup) both call it, so the order
// of every fp32 sum -- and with it the bits of a row -- cannot differ between the two.
#pragma once

#include "common.hpp"

#include <climits>

namespace sdfr {

// torch.relu keeps NaN (fmaxf(NaN, 0) would return 0 and hide bad weights or points); the NaN returned is the
// canonical positive one, which the bit-pattern maximum of the set pooling carries to the output
static __device__ __forceinline__ float relu_nan(float v) { return (v != v) ? __int_as_float(0x7fc00000) : fmaxf(v, 0.0f); }

// an int that orders as the float does (negative floats too; -0 below +0); a NaN becomes the canonical positive one,
// above +inf.  INT_MIN is no float's key: "no row yet".
static __device__ __forceinline__ int order_key(float v) {
  if (v != v) return 0x7fc00000;
  const int b = __float_as_int(v);
  return b >= 0 ? b : b ^ 0x7fffffff;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
// (K = 128, the mug backbone's inner layers, as ONE chunk -- 66 KB of dynamic LDS, a run-time row stride -- was
// measured: 13.8 -> 16.7 us per layer; the second chunk's four columns cost less than that)
constexpr int kPtsPerBlock = 64, kColsPerBlock = 64, kChunk = 124;
// K runs in chunks of kChunk columns staged in LDS (X tile and W tile, rows padded by one float: a row stride of a
// multiple of 32 floats would put the 16 rows a wave-instruction reads into one bank)
constexpr int kTileLd = kChunk + 1;

// Rows [p0, p0 + 64) of one set, columns [blockIdx.y * 64, + 64), by a workgroup of 256 threads: a wave = 16 points x
// 64 columns (4 accumulator tiles).  Y = relu((X W^T + c) * s + t), optionally y = resid + Y, and
// colmax[col] = max(colmax[col], max over the tile's rows < `rows` of Y) -- or of resid + Y as order keys (pool_resid).
//   x [rows][ldx] (K = cin columns used), w [cout][ldw] (first cin columns used), cvec / bn_scale / bn_shift [cout]
//   xs, ws [64 * kTileLd], wave_max [4][64]: the caller's __shared__ arrays.  The caller puts a barrier between two
//   calls; every thread of the workgroup takes part (barriers inside).
//   pool_resid is a template parameter: chosen at run time, the order keys cost every layer's epilogue ~230 of 1370
//   instructions (batched forward on 32 x 2500 points: 646 -> 632 us).
//   own_acc: the four accumulator tiles are this function's own array, or (false) *kernel_acc, an array of the
//   calling kernel.  The same bits, two register allocations: the compiler finishes this function before it inlines
//   it, and only a kernel's own array stays one block of 16 accumulation registers.  Each layer kernel takes the form
//   it was measured faster with (us, LABNOTES 2026-10-20): single-set 128 -> 1024 over 21 k rows 108 own, 119 the
//   kernel's (111 before the two kernels shared this function); batched, 32 x 2500 rows, 354 own, 344 the kernel's
//   (352 before).
template <bool pool_resid, bool own_acc>
static __device__ __forceinline__ void pointnet_tile(
    float* xs, float* ws, int (*wave_max)[kColsPerBlock], f32x4 (*kernel_acc)[4], const float* __restrict__ x, int rows,
    int p0, int cin, int ldx, const float* __restrict__ w, int ldw, const float* __restrict__ cvec,
    const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, const float* __restrict__ resid,
    float* __restrict__ y, int ldy, int cout, int* __restrict__ colmax) {
  constexpr int ld = kTileLd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.y * kColsPerBlock;
  const int row = lane & 15, kq = lane >> 4;
  // (rows of X and W 16 bytes apart and aligned: the staging's vector form -- workgroup-uniform)
  const bool vec_ok = ((ldx | ldw) & 3) == 0 && (((uintptr_t)x | (uintptr_t)w) & 15) == 0;
  f32x4 own[4];
  f32x4 (&acc)[4] = own_acc ? own : *kernel_acc;
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const float* xa = xs + (wave * 16 + row) * ld + kq;
  const float* wb = ws + row * ld + kq;
  for (int kc = 0; kc < cin; kc += kChunk) {
    const int kn = min(kChunk, cin - kc), kp = (kn + 3) & ~3;  // this chunk, padded to the MFMA's 4
    if (kc) __syncthreads();
    if (vec_ok && (kn & 3) == 0) {
      // 16-byte loads, no division: thread -> (row tid / 4, vectors tid % 4, + 4, ...): four threads walk a row's 512
      // bytes 64 at a time, and eight loads (four of X, four of W) are in flight per thread before the first LDS store
      // (the element-wise form below: 124 dependent iterations of a divide, two 4-byte loads and two stores per thread
      // -- 27 us per 128 -> 128 layer over 21 k points, most of it here)
      const int r = tid >> 2, sub = tid & 3, kv = kn >> 2;
      const bool xr = p0 + r < rows, wr = c0 + r < cout;
      const f32x4* xg = reinterpret_cast<const f32x4*>(x + (size_t)(p0 + r) * ldx + kc);
      const f32x4* wg = reinterpret_cast<const f32x4*>(w + (size_t)(c0 + r) * ldw + kc);
      const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int v0 = sub; v0 < kv; v0 += 16) {
        f32x4 xv[4], wv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int v = v0 + 4 * u;
          xv[u] = (xr && v < kv) ? xg[v] : zero4;
          wv[u] = (wr && v < kv) ? wg[v] : zero4;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int v = v0 + 4 * u;
          if (v < kv) {
            float* xd = xs + r * ld + 4 * v;
            float* wd = ws + r * ld + 4 * v;
            xd[0] = xv[u].x; xd[1] = xv[u].y; xd[2] = xv[u].z; xd[3] = xv[u].w;
            wd[0] = wv[u].x; wd[1] = wv[u].y; wd[2] = wv[u].z; wd[3] = wv[u].w;
          }
        }
      }
    } else {
      for (int i = tid; i < kPtsPerBlock * kp; i += 256) {
        const int r = i / kp, k = i - r * kp;
        xs[r * ld + k] = (p0 + r < rows && k < kn) ? x[(size_t)(p0 + r) * ldx + kc + k] : 0.0f;
        ws[r * ld + k] = (c0 + r < cout && k < kn) ? w[(size_t)(c0 + r) * ldw + kc + k] : 0.0f;
      }
    }
    __syncthreads();
    for (int k0 = 0; k0 < kp; k0 += 4) {
      const float a = xa[k0];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wb[j * 16 * ld + k0], acc[j], 0, 0, 0);
    }
  }
  // epilogue: the accumulator holds D[point 4 * kq + r][column row] of each tile
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = c0 + j * 16 + row;
    const bool col_ok = col < cout;
    const float cv = col_ok ? cvec[col] : 0.0f, s = col_ok ? bn_scale[col] : 0.0f, t = col_ok ? bn_shift[col] : 0.0f;
    // ReLU output is >= 0 or NaN (torch's relu and max propagate NaN: pointnet.py:64-96); non-negative floats
    // order as ints and the canonical positive NaN lies above +inf, so the set maximum is taken on the bit patterns.
    // pool_resid (a residual link into the LAST layer): the pooled resid + Y may be negative -- order keys
    int vmax = pool_resid ? INT_MIN : 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = p0 + wave * 16 + kq * 4 + r;
      const float v = relu_nan(fmaf(acc[j][r] + cv, s, t));
      if (p < rows && col_ok) {
        const float o = resid ? resid[(size_t)p * ldy + col] + v : v;
        if (y) y[(size_t)p * ldy + col] = o;
        vmax = max(vmax, pool_resid ? order_key(o) : __float_as_int(v));
      }
    }
    vmax = max(vmax, __shfl_xor(vmax, 16, 64));
    vmax = max(vmax, __shfl_xor(vmax, 32, 64));
    if (kq == 0) wave_max[wave][j * 16 + row] = vmax;
  }
  __syncthreads();
  if (tid < kColsPerBlock && c0 + tid < cout)
    atomicMax(&colmax[c0 + tid], max(max(wave_max[0][tid], wave_max[1][tid]), max(wave_max[2][tid], wave_max[3][tid])));
}

}  // namespace sdfr
