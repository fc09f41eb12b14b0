// annotate.hip -- the visibility mask of an annotated frame (sdfr_visible_mask), gfx950.
//
// What the reference's AnnotatedRedwoodDataset._compute_mask does with three boolean tensor passes and an indexed
// assignment (initialization/datasets/redwood_dataset.py:262-275): a pixel belongs to the object where the posed
// ground-truth mesh covers it (rendered != 0) unless the sensor saw something closer than the mesh by more than
// `margin` there (observed != 0 && observed < rendered - margin).  B images per call.
//
// Launch sequence (integer atomics only, no allocation, no host synchronisation):
//   1. zero_words_kernel (B * 4 / 256)            -- counts := 0, only when counts are asked for
//   2. visible_mask_kernel (ceil(n / 1024), B)    -- one workgroup of 256 lanes takes 1024 pixels of one image
// A streaming pass: 8 bytes read and 1 to 5 written per pixel.  Image b starts at pixel b * n of every buffer, so its
// first pixel may sit at any 4-byte boundary (a view into a larger buffer; n no multiple of 4).  Per image the kernel
// therefore peels `head` pixels, 0 to 3, up to the first 16-byte boundary of `rendered`; behind them every lane takes
// four consecutive pixels with one 16-byte load per input, one 4-byte store of the mask and one 16-byte store of
// `masked`, and the up to three pixels left at the end are single again.  That form needs `observed` (and `masked`)
// to be as far from a 16-byte boundary as `rendered`, and the mask's byte at pixel `head` to sit at a 4-byte boundary;
// an image for which that does not hold is walked pixel by pixel, coalesced.  The choice is uniform over a workgroup.
// The counts of a workgroup are summed in a wave (four 16-bit fields of one 64-bit word), across its waves in LDS, and
// added with four integer atomics: the same bits on every run.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "common.hpp"

#pragma clang fp contract(off)

namespace sdfr {
namespace {

constexpr int kMaskThreads = 256;
constexpr int kMaskPixels = 4 * kMaskThreads;   // pixels per workgroup

// bit 0: visible, and the pixel's counts as 16-bit fields from bit 16 on (covered | visible | occluded | valid)
__device__ __forceinline__ unsigned long long mask_pixel(float r, float o, float margin, bool& visible) {
  const bool covered = r != 0.0f;
  const bool occluded = covered && (o != 0.0f && o < r - margin);
  visible = covered && !occluded;
  const bool valid = visible && o != 0.0f;
  return (unsigned long long)covered | ((unsigned long long)visible << 16) | ((unsigned long long)occluded << 32) |
         ((unsigned long long)valid << 48);
}

__global__ void __launch_bounds__(kMaskThreads) visible_mask_kernel(const float* __restrict__ rendered,
                                                                    const float* observed, long long n, float margin,
                                                                    unsigned char* __restrict__ mask, float* masked,
                                                                    int* __restrict__ counts) {
  const int b = blockIdx.y;
  const float* r_img = rendered + (size_t)b * n;
  const float* o_img = observed + (size_t)b * n;
  unsigned char* m_img = mask + (size_t)b * n;
  float* d_img = masked ? masked + (size_t)b * n : nullptr;

  // pixels in front of rendered's first 16-byte boundary (the pointers are 4-byte aligned: checked by the caller)
  long long head = (long long)(((16u - (unsigned)((uintptr_t)r_img & 15u)) & 15u) >> 2);
  head = head < n ? head : n;
  const bool wide = ((uintptr_t)o_img & 15u) == ((uintptr_t)r_img & 15u) &&
                    (!d_img || ((uintptr_t)d_img & 15u) == ((uintptr_t)r_img & 15u)) &&
                    (((uintptr_t)m_img + (uintptr_t)head) & 3u) == 0;
  unsigned long long sum = 0;
  if (wide) {   // uniform over the workgroup
    const long long groups = (n - head) >> 2;
    const long long g = (long long)blockIdx.x * kMaskThreads + threadIdx.x;
    if (g < groups) {
      const long long i = head + 4 * g;
      const float4 r = *reinterpret_cast<const float4*>(r_img + i);
      const float4 o = *reinterpret_cast<const float4*>(o_img + i);
      bool v0, v1, v2, v3;
      sum = mask_pixel(r.x, o.x, margin, v0) + mask_pixel(r.y, o.y, margin, v1) + mask_pixel(r.z, o.z, margin, v2) +
            mask_pixel(r.w, o.w, margin, v3);
      *reinterpret_cast<unsigned*>(m_img + i) =
          (unsigned)v0 | ((unsigned)v1 << 8) | ((unsigned)v2 << 16) | ((unsigned)v3 << 24);
      if (d_img)
        *reinterpret_cast<float4*>(d_img + i) =
            make_float4(v0 ? o.x : 0.0f, v1 ? o.y : 0.0f, v2 ? o.z : 0.0f, v3 ? o.w : 0.0f);
    }
    // the pixels in front of the first group and behind the last one, at most three each: workgroup 0, lanes 0 - 5
    if (blockIdx.x == 0 && threadIdx.x < 6) {
      const long long tail0 = head + 4 * groups;
      const long long i = threadIdx.x < 3 ? (long long)threadIdx.x : tail0 + (threadIdx.x - 3);
      if (threadIdx.x < 3 ? i < head : i < n) {
        const float o = o_img[i];
        bool v;
        sum += mask_pixel(r_img[i], o, margin, v);
        m_img[i] = (unsigned char)v;
        if (d_img) d_img[i] = v ? o : 0.0f;
      }
    }
  } else {
    const long long first = (long long)blockIdx.x * kMaskPixels + threadIdx.x;
#pragma unroll
    for (int u = 0; u < kMaskPixels / kMaskThreads; ++u) {
      const long long i = first + u * kMaskThreads;
      if (i < n) {
        const float o = o_img[i];
        bool v;
        sum += mask_pixel(r_img[i], o, margin, v);
        m_img[i] = (unsigned char)v;
        if (d_img) d_img[i] = v ? o : 0.0f;
      }
    }
  }
  if (!counts) return;   // uniform
  // a lane adds at most 5 per field, a workgroup at most 4 * 256 + 6: the 16-bit fields never carry
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
  __shared__ unsigned long long s_sum[kMaskThreads / 64];
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < kMaskThreads / 64; ++w) total += s_sum[w];
    const int field = (int)((total >> (16 * threadIdx.x)) & 0xffffu);
    if (field) atomicAdd(counts + 4 * b + threadIdx.x, field);   // integers: no order of arrival in the result
  }
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" int sdfr_visible_mask(const float* rendered, const float* observed, int B, int H, int W, float margin,
                                 unsigned char* mask, float* masked, int* counts, int device, void* stream) {
  const char* fn = "sdfr_visible_mask";
  if (B < 0 || B > 65535) return fail(SDFR_E_INVALID, "%s: B=%d out of range [0,65535]", fn, B);
  if (H < 1 || W < 1) return fail(SDFR_E_INVALID, "%s: image size H=%d, W=%d must be >= 1", fn, H, W);
  if ((long long)H * W > INT_MAX)
    return fail(SDFR_E_INVALID, "%s: H=%d x W=%d pixels exceed an int32 count", fn, H, W);
  if (!(margin >= 0.0f) || !(margin < INFINITY))
    return fail(SDFR_E_INVALID, "%s: margin=%g must be >= 0 and finite", fn, (double)margin);
  if (B == 0) return 0;
  if (!rendered || !observed || !mask)
    return fail(SDFR_E_NULL, "%s: NULL pointer argument (only masked and counts may be NULL)", fn);
  if (((uintptr_t)rendered | (uintptr_t)observed | (uintptr_t)masked | (uintptr_t)counts) & 3u)
    return fail(SDFR_E_INVALID, "%s: rendered, observed, masked and counts must be 4-byte aligned", fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)H * W;
  if (counts) zero_words_async(reinterpret_cast<float*>(counts), (size_t)B * 4, st);   // overwritten, never accumulated
  // (the wide form's groups start behind `head` pixels: n / 4 groups at most, and its workgroup 0 takes the rest)
  hipLaunchKernelGGL(visible_mask_kernel, dim3((unsigned)((n + kMaskPixels - 1) / kMaskPixels), (unsigned)B),
                     dim3(kMaskThreads), 0, st, rendered, observed, n, margin, mask, masked, counts);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
