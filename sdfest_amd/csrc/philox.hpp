// philox.hpp -- Philox-4x32-10 (Salmon et al., SC'11), the Random123 round function and Weyl key schedule, shared by
// metrics.hip (surface sampling), encoder.hip and vae_train.hip (the VAE's normal noise).  tests/metrics_twin.py
// restates it in numpy.
#pragma once

#include <hip/hip_runtime.h>

namespace sdfr {

struct U4 {
  unsigned x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c.x;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c.z;
    const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0;
    const unsigned hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
    c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// The VAE's normal noise eps[i][j] (include/sdfr.h, group 7): Box-Muller in fp64 on the words of counter {i, j, 0,
// kNoiseStream}, rounded to fp32 once.  One function for the encoder's forward and the trainer's forward and backward
// (encoder.hip, vae_train.hip): the three see the same eps for a seed.
constexpr unsigned kNoiseStream = 0x56414531u;  // counter word 3: the encoder's stream ("VAE1"), apart from metrics.hip
__device__ __forceinline__ float normal_eps(unsigned long long seed, unsigned i, unsigned j) {
  const U4 r = philox4x32_10(U4{i, j, 0u, kNoiseStream}, (unsigned)seed, (unsigned)(seed >> 32));
  const double u1 = ((double)(r.x >> 5) * 67108864.0 + (double)(r.y >> 6)) * (1.0 / 9007199254740992.0);
  const double u2 = ((double)(r.z >> 5) * 67108864.0 + (double)(r.w >> 6)) * (1.0 / 9007199254740992.0);
  return (float)(sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2));
}

}  // namespace sdfr
