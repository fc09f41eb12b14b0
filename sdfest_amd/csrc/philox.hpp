// philox.hpp -- Philox-4x32-10 (Salmon et al., SC'11), the Random123 round function and Weyl key schedule, shared by
// metrics.hip (surface sampling) and encoder.hip (the VAE's normal noise).  tests/metrics_twin.py restates it in numpy.
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

}  // namespace sdfr
