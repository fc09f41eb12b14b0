// shade.hip -- looking at a render, gfx950: surface normals at the hit points of a depth image (sdfr_render_normals),
// the range of its hit depths (sdfr_depth_range) and packed RGB8 images of it -- colour-mapped depth, colour-mapped
// error against a target, Lambert shading (sdfr_shade_frames).
//
// The normal.  A pixel of depth z != 0 has the hit point of the backward (device.hpp: hit_point) and its cell
// (gather_cell: the same clamped base and the same un-clamped offsets, cells that extrapolate past the grid included).
// The gradient of the trilinear interpolant at the offsets (ox, oy, oz), from the corners v[4 ix + 2 iy + iz], is
//   g.x = sum_{iy,iz} w_y(iy) w_z(iz) (v[1,iy,iz] - v[0,iy,iz]),   w(0) = 1 - o, w(1) = o,
// g.y and g.z likewise; the grid is uniform and inv_scale > 0, so g has the direction of the object-frame gradient and
// R g / |g| is the unit normal in the camera frame, pointing away from the object (the SDF is positive outside).
// surface_normal() is the ONE statement of it: the normal map and the shaded image call it.
//
// sdfr_shade_frames is one pass over the pixels of B frames, bound by memory traffic: per pixel it reads 4 (depth) + 4
// (target) bytes and writes 3 x 3, and the shaded image adds four 8-byte gathers of the grid per hit pixel, which the
// L2 serves.  A lane takes kShadePx = 4 ADJACENT pixels of the frame's row-major pixel stream (a group may run over the
// end of an image row): 12 output bytes = three whole dwords per image, one 16-byte load per input.  That PACKED form
// needs H W to be a multiple of 4 and the buffers aligned (inputs 16, outputs 4 bytes); any other call takes the same
// kernel with per-pixel loads and single-byte stores, and with it the tail of a frame whose pixel count is odd.
// Every output byte is written, there are no atomics, and a frame's bytes depend on nothing but that frame's inputs.
#include <hip/hip_runtime.h>

#include <cmath>

#include "colormap_table.hpp"
#include "common.hpp"
#include "device.hpp"

namespace sdfr {
namespace {

constexpr int kShadeThreads = 256;
constexpr int kShadePx = SDFR_SHADE_PIXELS_PER_LANE;
constexpr int kRangeThreads = SDFR_RANGE_THREADS;
static_assert(kShadePx == 4, "the packed store form is written for four pixels = three dwords per lane");
static_assert(kRangeThreads % 64 == 0 && kRangeThreads <= 1024, "whole waves, one workgroup");

// the part of a view's record that hit_point and rot_f read, in the expressions of the renderer's set-up
// (render.hip, setup_pose): the same rotation and the same e = R^T p
__device__ __forceinline__ void shade_pose(int b, const float* __restrict__ pos, const float* __restrict__ quat,
                                           const float* __restrict__ inv_scale, ViewSetup& s) {
  const float x = quat[4 * b], y = quat[4 * b + 1], z = quat[4 * b + 2], w = quat[4 * b + 3];
  const V3 p = mk(pos[3 * b], pos[3 * b + 1], pos[3 * b + 2]);
  s.rot[0] = 1 - 2 * (y * y + z * z); s.rot[1] = 2 * (x * y - w * z);     s.rot[2] = 2 * (x * z + w * y);
  s.rot[3] = 2 * (x * y + w * z);     s.rot[4] = 1 - 2 * (x * x + z * z); s.rot[5] = 2 * (y * z - w * x);
  s.rot[6] = 2 * (x * z - w * y);     s.rot[7] = 2 * (y * z + w * x);     s.rot[8] = 1 - 2 * (x * x + y * y);
  s.e[0] = s.rot[0] * p.x + s.rot[3] * p.y + s.rot[6] * p.z;
  s.e[1] = s.rot[1] * p.x + s.rot[4] * p.y + s.rot[7] * p.z;
  s.e[2] = s.rot[2] * p.x + s.rot[5] * p.y + s.rot[8] * p.z;
  s.isc = inv_scale[b];
}

// Unit normal in the camera frame at the hit point of pixel (row, col) of depth z != 0; three zeros where the gradient
// vanishes or is not finite.  The gradient is divided by its largest component first, so that neither a tiny nor a huge
// one is lost to the squares of the length.
__device__ __forceinline__ V3 surface_normal(const ViewSetup& s, const float* __restrict__ vol, int R, int row, int col,
                                             float z, float cx, float cy, float rfx, float rfy) {
  const float h = 0.5f * (float)(R - 1);
  const HitPoint hp = hit_point(s, row, col, z, cx, cy, rfx, rfy, s.isc, h);
  Cell c;
  gather_cell<0>(vol, R, hp.gx, hp.gy, hp.gz, c);   // (the cell is clamped into the grid whatever z holds)
  const float ax = 1.0f - c.ox, ay = 1.0f - c.oy, az = 1.0f - c.oz;
  const float gx = fmaf(ay * az, c.v[4] - c.v[0], fmaf(ay * c.oz, c.v[5] - c.v[1],
                   fmaf(c.oy * az, c.v[6] - c.v[2], (c.oy * c.oz) * (c.v[7] - c.v[3]))));
  const float gy = fmaf(ax * az, c.v[2] - c.v[0], fmaf(ax * c.oz, c.v[3] - c.v[1],
                   fmaf(c.ox * az, c.v[6] - c.v[4], (c.ox * c.oz) * (c.v[7] - c.v[5]))));
  const float gz = fmaf(ax * ay, c.v[1] - c.v[0], fmaf(ax * c.oy, c.v[3] - c.v[2],
                   fmaf(c.ox * ay, c.v[5] - c.v[4], (c.ox * c.oy) * (c.v[7] - c.v[6]))));
  const float m = fmaxf(fabsf(gx), fmaxf(fabsf(gy), fabsf(gz)));
  if (!(m > 0.0f) || !(m < INFINITY) || gx != gx || gy != gy || gz != gz) return mk(0.0f, 0.0f, 0.0f);
  const float rm = 1.0f / m;
  const V3 u = mk(gx * rm, gy * rm, gz * rm);
  const float inv_len = 1.0f / sqrtf(dot(u, u));   // 1 <= |u|^2 <= 3
  return rot_f(s, inv_len * u);
}

// grid: (ceil(H W / 256), B): one pixel per thread
__global__ __launch_bounds__(kShadeThreads) void render_normals_kernel(
    const float* __restrict__ depth, const float* __restrict__ sdf, int R, long long sdf_view_stride,
    const float* __restrict__ pos, const float* __restrict__ quat, const float* __restrict__ inv_scale, int W, int HW,
    float cx, float cy, float rfx, float rfy, float* __restrict__ normals) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * kShadeThreads + threadIdx.x;
  if (p >= HW) return;
  const size_t at = (size_t)b * HW + p;
  const float z = depth[at];
  V3 n = mk(0.0f, 0.0f, 0.0f);
  if (z != 0.0f) {
    ViewSetup s;
    shade_pose(b, pos, quat, inv_scale, s);
    const int row = p / W, col = p - row * W;
    n = surface_normal(s, sdf + (size_t)b * sdf_view_stride, R, row, col, z, cx, cy, rfx, rfy);
  }
  float* out = normals + 3 * at;
  out[0] = n.x; out[1] = n.y; out[2] = n.z;
}

// ---- range ----------------------------------------------------------------------------------------------------------
// grid: the number of range rows; workgroup r reduces `count` floats from depth + r * count.  Minimum and maximum do
// not depend on the order of their operands: the same bits whatever the workgroup's shape.
__global__ __launch_bounds__(kRangeThreads) void depth_range_kernel(const float* __restrict__ depth, long long count,
                                                                    float* __restrict__ range) {
  __shared__ float part[2][kRangeThreads / 64];
  const float* src = depth + (size_t)blockIdx.x * count;
  float lo = INFINITY, hi = -INFINITY;
  for (long long i = threadIdx.x; i < count; i += kRangeThreads) {
    const float z = src[i];
    if (z != 0.0f && fabsf(z) < INFINITY) {   // finite and non-zero (a NaN fails the comparison)
      lo = fminf(lo, z);
      hi = fmaxf(hi, z);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, 64));
    hi = fmaxf(hi, __shfl_xor(hi, off, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[0][wave] = lo; part[1][wave] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kRangeThreads / 64; ++w) {
      lo = fminf(lo, part[0][w]);
      hi = fmaxf(hi, part[1][w]);
    }
    const bool any = lo <= hi;
    range[2 * blockIdx.x] = any ? lo : 0.0f;
    range[2 * blockIdx.x + 1] = any ? hi : 0.0f;
  }
}

// ---- frames ---------------------------------------------------------------------------------------------------------
struct ShadeArgs {
  const float* depth;
  const float* sdf;
  const float* pos;
  const float* quat;
  const float* inv_scale;
  const float* target;
  const float* range;
  unsigned char* depth_rgb;
  unsigned char* error_rgb;
  unsigned char* shaded_rgb;
  long long sdf_view_stride;
  int R, W, HW, V, range_stride;
  float cx, cy, rfx, rfy;
  float error_max, ambient;
  float light[3], base[3];
  unsigned background;   // in memory order: R | G << 8 | B << 16
};

__device__ __forceinline__ unsigned memory_order(unsigned rgb) {   // 0xRRGGBB -> R | G << 8 | B << 16
  return ((rgb >> 16) & 0xffu) | (rgb & 0xff00u) | ((rgb & 0xffu) << 16);
}
// table entry clamp(floor(t), 0, 255) (a NaN takes entry 0)
__device__ __forceinline__ unsigned lookup(const unsigned* __restrict__ table, float t) {
  return table[(int)fminf(fmaxf(floorf(t), 0.0f), (float)(kColormapEntries - 1))];
}
__device__ __forceinline__ unsigned channel(float base, float s) {
  return (unsigned)(int)rintf(255.0f * fminf(fmaxf(base * s, 0.0f), 1.0f));
}
struct __attribute__((packed, aligned(4))) Rgb4 {   // four RGB8 pixels: 12-byte store at 4-byte alignment
  unsigned a, b, c;
};
template <bool PACKED>
__device__ __forceinline__ void store_pixels(unsigned char* __restrict__ image, size_t first, int n,
                                             const unsigned (&c)[kShadePx]) {
  unsigned char* out = image + 3 * first;
  if (PACKED) {
    *reinterpret_cast<Rgb4*>(out) = Rgb4{c[0] | (c[1] << 24), (c[1] >> 8) | (c[2] << 16), (c[2] >> 16) | (c[3] << 8)};
  } else {
    for (int k = 0; k < n; ++k) {
      out[3 * k] = (unsigned char)(c[k] & 0xffu);
      out[3 * k + 1] = (unsigned char)((c[k] >> 8) & 0xffu);
      out[3 * k + 2] = (unsigned char)((c[k] >> 16) & 0xffu);
    }
  }
}

// grid: (ceil(ceil(H W / 4) / 256), B): lane -> pixels 4 g .. 4 g + 3 of frame blockIdx.y
template <bool PACKED>
__global__ __launch_bounds__(kShadeThreads) void shade_frames_kernel(const ShadeArgs a) {
  __shared__ unsigned table[kColormapEntries];
  static_assert(kColormapEntries == kShadeThreads, "one table entry per thread");
  table[threadIdx.x] = memory_order(kViridisRGB[threadIdx.x]);
  __syncthreads();
  const int f = blockIdx.y;
  const int p0 = (blockIdx.x * kShadeThreads + threadIdx.x) * kShadePx;
  if (p0 >= a.HW) return;
  const int n = min(kShadePx, a.HW - p0);   // PACKED: always kShadePx
  const size_t first = (size_t)f * a.HW + p0;

  float z[kShadePx], tg[kShadePx];
  if (PACKED) {
    const float4 z4 = *reinterpret_cast<const float4*>(a.depth + first);
    z[0] = z4.x; z[1] = z4.y; z[2] = z4.z; z[3] = z4.w;
  } else {
    for (int k = 0; k < kShadePx; ++k) z[k] = k < n ? a.depth[first + k] : 0.0f;
  }
  unsigned c[kShadePx];

  if (a.depth_rgb) {
    const float vmin = a.range[(size_t)f * a.range_stride], vmax = a.range[(size_t)f * a.range_stride + 1];
    const float span = vmax - vmin;
#pragma unroll
    for (int k = 0; k < kShadePx; ++k)
      c[k] = z[k] == 0.0f ? a.background : (vmax == vmin ? table[0] : lookup(table, (z[k] - vmin) / span * 256.0f));
    store_pixels<PACKED>(a.depth_rgb, first, n, c);
  }

  if (a.error_rgb) {
    const size_t tfirst = (size_t)(f % a.V) * a.HW + p0;
    if (PACKED) {
      const float4 t4 = *reinterpret_cast<const float4*>(a.target + tfirst);
      tg[0] = t4.x; tg[1] = t4.y; tg[2] = t4.z; tg[3] = t4.w;
    } else {
      for (int k = 0; k < kShadePx; ++k) tg[k] = k < n ? a.target[tfirst + k] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < kShadePx; ++k)
      c[k] = (z[k] == 0.0f || tg[k] == 0.0f) ? a.background
                                             : lookup(table, fabsf(z[k] - tg[k]) / a.error_max * 256.0f);
    store_pixels<PACKED>(a.error_rgb, first, n, c);
  }

  if (a.shaded_rgb) {
    ViewSetup s;
    shade_pose(f, a.pos, a.quat, a.inv_scale, s);
    int row = p0 / a.W, col = p0 - row * a.W;
    const float* vol = a.sdf + (size_t)(a.sdf_view_stride ? f / a.V : 0) * a.sdf_view_stride;
#pragma unroll
    for (int k = 0; k < kShadePx; ++k) {
      c[k] = a.background;
      if (z[k] != 0.0f) {
        const V3 nrm = surface_normal(s, vol, a.R, row, col, z[k], a.cx, a.cy, a.rfx, a.rfy);
        const float lambert = fmaxf(0.0f, fmaf(nrm.x, a.light[0], fmaf(nrm.y, a.light[1], nrm.z * a.light[2])));
        const float shade = fmaf(1.0f - a.ambient, lambert, a.ambient);
        c[k] = channel(a.base[0], shade) | (channel(a.base[1], shade) << 8) | (channel(a.base[2], shade) << 16);
      }
      if (++col == a.W) { col = 0; ++row; }
    }
    store_pixels<PACKED>(a.shaded_rgb, first, n, c);
  }
}

// the checks the three entries share; 0 or the code to return
int check_image(const char* fn, int B, int W, int H) {
  if (B <= 0 || W <= 0 || H <= 0) return fail(SDFR_E_INVALID, "%s: B=%d, W=%d, H=%d must be positive", fn, B, W, H);
  if (B > 65535) return fail(SDFR_E_INVALID, "%s: B=%d out of range [1,65535]", fn, B);
  if ((long long)W * H > (1ll << 30)) return fail(SDFR_E_INVALID, "%s: W*H=%lld exceeds 2^30", fn, (long long)W * H);
  return 0;
}
int check_grid(const char* fn, int R, long long sdf_view_stride) {
  if (R < 2 || R > 1024) return fail(SDFR_E_INVALID, "%s: R=%d out of range [2,1024]", fn, R);
  if (sdf_view_stride != 0 && sdf_view_stride < (long long)R * R * R)
    return fail(SDFR_E_INVALID, "%s: sdf_view_stride=%lld must be 0 (one shared grid) or >= R^3", fn, sdf_view_stride);
  return 0;
}
bool aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" int sdfr_render_normals(const float* depth, const float* sdf, int R, long long sdf_view_stride,
                                   const float* pos, const float* quat, const float* inv_scale, int B, int W, int H,
                                   float cx, float cy, float fx, float fy, float* normals, int device, void* stream) {
  const char* fn = "sdfr_render_normals";
  if (int rc = check_image(fn, B, W, H)) return rc;
  if (int rc = check_grid(fn, R, sdf_view_stride)) return rc;
  if (!depth || !sdf || !pos || !quat || !inv_scale || !normals) return fail(SDFR_E_INVALID, "%s: NULL pointer argument", fn);
  if (!aligned(depth, 4) || !aligned(sdf, 4) || !aligned(pos, 4) || !aligned(quat, 4) || !aligned(inv_scale, 4) ||
      !aligned(normals, 4))
    return fail(SDFR_E_INVALID, "%s: every buffer must be 4-byte aligned", fn);
  if (!(fx != 0.0f) || !(fy != 0.0f)) return fail(SDFR_E_INVALID, "%s: fx=%g, fy=%g must be non-zero", fn, (double)fx, (double)fy);
  SDFR_HIP_TRY(hipSetDevice(device));
  const int HW = W * H;
  const float rfx = (float)(1.0 / (double)fx), rfy = (float)(1.0 / (double)fy);
  hipLaunchKernelGGL(render_normals_kernel, dim3((HW + kShadeThreads - 1) / kShadeThreads, B), dim3(kShadeThreads), 0,
                     (hipStream_t)stream, depth, sdf, R, sdf_view_stride, pos, quat, inv_scale, W, HW, cx, cy, rfx, rfy,
                     normals);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_depth_range(const float* depth, int B, int W, int H, int shared, float* range, int device,
                                void* stream) {
  const char* fn = "sdfr_depth_range";
  if (int rc = check_image(fn, B, W, H)) return rc;
  if (!depth || !range) return fail(SDFR_E_INVALID, "%s: NULL pointer argument", fn);
  if (!aligned(depth, 4) || !aligned(range, 4)) return fail(SDFR_E_INVALID, "%s: depth and range must be 4-byte aligned", fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  const long long HW = (long long)W * H;
  hipLaunchKernelGGL(depth_range_kernel, dim3(shared ? 1 : B), dim3(kRangeThreads), 0, (hipStream_t)stream, depth,
                     shared ? HW * B : HW, range);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_shade_frames(const float* depth, const float* sdf, int R, long long sdf_view_stride,
                                 const float* pos, const float* quat, const float* inv_scale, int B, int W, int H,
                                 float cx, float cy, float fx, float fy, int views_per_state, const float* target,
                                 const float* range, int range_stride, float error_max, float light_x, float light_y,
                                 float light_z, float ambient, float base_r, float base_g, float base_b, int background,
                                 unsigned char* depth_rgb, unsigned char* error_rgb, unsigned char* shaded_rgb,
                                 int device, void* stream) {
  const char* fn = "sdfr_shade_frames";
  if (int rc = check_image(fn, B, W, H)) return rc;
  if (int rc = check_grid(fn, R, sdf_view_stride)) return rc;
  const int V = views_per_state;
  if (V < 1 || B % V != 0)
    return fail(SDFR_E_INVALID, "%s: views_per_state=%d must be >= 1 and divide B=%d", fn, V, B);
  if (!(error_max > 0.0f)) return fail(SDFR_E_INVALID, "%s: error_max=%g must be > 0", fn, (double)error_max);
  if (range_stride != 0 && range_stride != 2)
    return fail(SDFR_E_INVALID, "%s: range_stride=%d must be 0 (one range) or 2 (one per frame)", fn, range_stride);
  if (background < 0 || background > 0xffffff)
    return fail(SDFR_E_INVALID, "%s: background=0x%x must be 0xRRGGBB", fn, (unsigned)background);
  const double ll = std::sqrt((double)light_x * light_x + (double)light_y * light_y + (double)light_z * light_z);
  if (!(ll > 0.0) || !std::isfinite(ll) || !std::isfinite(ambient) || !std::isfinite(base_r) || !std::isfinite(base_g) ||
      !std::isfinite(base_b))
    return fail(SDFR_E_INVALID, "%s: light must be a finite non-zero direction, ambient and base_rgb finite", fn);
  if (!depth) return fail(SDFR_E_INVALID, "%s: depth is NULL", fn);
  if (!depth_rgb && !error_rgb && !shaded_rgb) return fail(SDFR_E_INVALID, "%s: all three outputs are NULL", fn);
  if (depth_rgb && !range) return fail(SDFR_E_INVALID, "%s: depth_rgb needs range", fn);
  if (error_rgb && !target) return fail(SDFR_E_INVALID, "%s: error_rgb needs target", fn);
  if (shaded_rgb && (!sdf || !pos || !quat || !inv_scale))
    return fail(SDFR_E_INVALID, "%s: shaded_rgb needs sdf, pos, quat and inv_scale", fn);
  if (!aligned(depth, 4) || !aligned(target, 4) || !aligned(range, 4) || !aligned(sdf, 4) || !aligned(pos, 4) ||
      !aligned(quat, 4) || !aligned(inv_scale, 4))
    return fail(SDFR_E_INVALID, "%s: every float buffer must be 4-byte aligned", fn);
  if (!(fx != 0.0f) || !(fy != 0.0f)) return fail(SDFR_E_INVALID, "%s: fx=%g, fy=%g must be non-zero", fn, (double)fx, (double)fy);
  SDFR_HIP_TRY(hipSetDevice(device));
  ShadeArgs a;
  a.depth = depth; a.sdf = sdf; a.pos = pos; a.quat = quat; a.inv_scale = inv_scale; a.target = target; a.range = range;
  a.depth_rgb = depth_rgb; a.error_rgb = error_rgb; a.shaded_rgb = shaded_rgb;
  a.sdf_view_stride = sdf_view_stride;
  a.R = R; a.W = W; a.HW = W * H; a.V = V; a.range_stride = range_stride;
  a.cx = cx; a.cy = cy; a.rfx = (float)(1.0 / (double)fx); a.rfy = (float)(1.0 / (double)fy);
  a.error_max = error_max; a.ambient = ambient;
  a.light[0] = (float)(light_x / ll); a.light[1] = (float)(light_y / ll); a.light[2] = (float)(light_z / ll);
  a.base[0] = base_r; a.base[1] = base_g; a.base[2] = base_b;
  const unsigned bg = (unsigned)background;
  a.background = ((bg >> 16) & 0xffu) | (bg & 0xff00u) | ((bg & 0xffu) << 16);
  const bool packed = a.HW % kShadePx == 0 && aligned(depth, 16) && aligned(target, 16) && aligned(depth_rgb, 4) &&
                      aligned(error_rgb, 4) && aligned(shaded_rgb, 4);
  const int groups = (a.HW + kShadePx - 1) / kShadePx;
  const dim3 grid((groups + kShadeThreads - 1) / kShadeThreads, B);
  if (packed) hipLaunchKernelGGL(shade_frames_kernel<true>, grid, dim3(kShadeThreads), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(shade_frames_kernel<false>, grid, dim3(kShadeThreads), 0, (hipStream_t)stream, a);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
