// information_gram.hpp -- what the 32-wide information kernels share, each piece stated once: the F x F Gram product of a
// wave's 64 feature rows on the matrix cores (render_information_shape_kernel in information.hip, pc_information_kernel
// in pc_information.hip) and the latent features of a located cell.
//
// The Gram product.  A Gram matrix is the GEMM F^T F with K = rows (pixels or points).  F = 10 + T <= 32, so one
// v_mfma_f32_32x32x2_f32 block holds it: lane l holds A[l & 31][l >> 5] and B[l >> 5][l & 31], and with A = F^T, B = F
// both are the SAME register, feature l & 31 of row 2 g + (l >> 5) of k-step g -- word 64 g + l of the wave's [row][32]
// block in LDS, 32 MFMAs per 64 rows into 16 accumulator registers.  The alternative, three 16 x 16 x 4 products on a low
// and a high half of the features (low x low, low x high, high x high), would issue 48 MFMAs of half the cycles per 64
// rows -- three quarters of the matrix-core time -- but needs two operand reads per step, three accumulators and the
// low x high block mirrored by hand to keep (i, j) and (j, i) the same bits.  The kernels' time is in the gathers of a
// row's features, not in 32 MFMAs per 64 rows, so the form with one read, one instruction and one layout per step is the
// one built.  The instruction is a k-ordered fma chain with one rounding per product, so the sums have ONE order -- the
// same bits on every run -- and entry (i, j) and entry (j, i) see the same products in the same order: the matrix is
// symmetric bit for bit.  A row that takes no part is all zeros (never a product with a possibly non-finite derivative),
// a row that does has 1 as its last feature: entry (F - 1, F - 1) is the exact count.
#pragma once
#include "device.hpp"

namespace sdfr {
namespace {

constexpr int kGramF = 32;      // feature slots of a row
constexpr int kGramWaves = 4;   // waves of a workgroup, each with a block of its own
static_assert(10 + SDFR_INFO_MAX_TANGENTS <= kGramF, "a row holds d0 .. d7, the tangents, r and 1");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// a wave's block: [row][feature], features F .. 31 zero; the wave's 32 x 32 result (row-major) overlays it at the end
struct GramBlock {
  float w[64 * kGramF];
};

// A wave reads back across lanes what its own lanes wrote: the LDS serves a wave's accesses in order; the fences keep
// the compiler from moving them and wait for the writes.  No workgroup barrier: the block is the wave's own.
__device__ __forceinline__ void gram_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// acc += the Gram matrix of the wave's 64 rows, f the lane's.  (The next call's rows go into the same block: behind
// these reads, hence the second sync.)
__device__ __forceinline__ void gram32_accumulate(const float (&f)[kGramF], GramBlock& blk, int lane, f32x16& acc) {
  f32x4* mine = reinterpret_cast<f32x4*>(blk.w + lane * kGramF);
#pragma unroll
  for (int k = 0; k < kGramF / 4; ++k) mine[k] = f32x4{f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]};
  gram_wave_sync();
#pragma unroll 8
  for (int g = 0; g < 32; ++g) {
    const float x = blk.w[64 * g + lane];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x, x, acc, 0, 0, 0);
  }
  gram_wave_sync();
}

// C/D layout: column = lane & 31, row = (register & 3) + 8 (register >> 2) + 4 (lane >> 5); into the wave's own block.
// (acc by value and the lane's part of the address formed once: the registers and paired LDS stores of the kernels that
// had these statements in their own bodies; by reference each store kept an address register of its own)
__device__ __forceinline__ void gram32_store(f32x16 acc, GramBlock& blk, int lane) {
  float* mine = blk.w + 4 * (lane >> 5) * 32 + (lane & 31);
#pragma unroll
  for (int k = 0; k < 16; ++k) mine[((k & 3) + 8 * (k >> 2)) * 32] = acc[k];
}

// the F x F record: the four waves' blocks summed as (0 + 1) + (2 + 3); behind a __syncthreads() after gram32_store
__device__ __forceinline__ void gram32_record(const GramBlock (&blk)[kGramWaves], int F, int tid, float* __restrict__ rec) {
  for (int e = tid; e < F * F; e += 64 * kGramWaves) {
    const int w = (e / F) * 32 + e % F;
    rec[e] = (blk[0].w[w] + blk[1].w[w]) + (blk[2].w[w] + blk[3].w[w]);
  }
}

// The T latent features of a row into f[8 ..]: weight * trilerp (x, then y, then z) of the eight corners of jac at the
// cell gather_cell located, with its offsets.  jac is voxel-major for this: the T tangents of a grid corner are Tp / 4
// 16-byte loads.
__device__ __forceinline__ void latent_features(const Cell& c, const float* __restrict__ jac, int Tp, int T, int Rr,
                                                float weight, float (&f)[kGramF]) {
  const float ox = c.ox, oy = c.oy, oz = c.oz;
  const float ax = 1.0f - ox, ay = 1.0f - oy, az = 1.0f - oz;
  const float* base = jac + (size_t)c.lin * Tp;
  const size_t sy = (size_t)Rr * Tp, sx = (size_t)Rr * Rr * Tp;
#pragma unroll
  for (int g = 0; g < (SDFR_INFO_MAX_TANGENTS + 3) / 4; ++g) {
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
      if (8 + 4 * g + j < kGramF) f[8 + 4 * g + j] = 4 * g + j < T ? weight * tri : 0.0f;
    }
  }
}

}  // namespace
}  // namespace sdfr
