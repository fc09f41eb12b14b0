// initnet_tile.hpp -- what the per-point layer kernels of the initialisation network share (initnet.hip: one set per
// launch; initnet_eval.hip: N sets per launch): the tile and the k chunk, which fix the order of every fp32 sum, so
// that the two give the same bits per row.
#pragma once

#include "common.hpp"

namespace sdfr {

// torch.relu keeps NaN (fmaxf(NaN, 0) would return 0 and hide bad weights or points); the NaN returned is the
// canonical positive one, which the bit-pattern maximum of the set pooling carries to the output
static __device__ __forceinline__ float relu_nan(float v) { return (v != v) ? __int_as_float(0x7fc00000) : fmaxf(v, 0.0f); }

typedef float f32x4 __attribute__((ext_vector_type(4)));
// (K = 128, the mug backbone's inner layers, as ONE chunk -- 66 KB of dynamic LDS, a run-time row stride -- was
// measured: 13.8 -> 16.7 us per layer; the second chunk's four columns cost less than that)
constexpr int kPtsPerBlock = 64, kColsPerBlock = 64, kChunk = 124;

}  // namespace sdfr
