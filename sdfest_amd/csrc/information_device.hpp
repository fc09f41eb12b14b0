// information_device.hpp -- the device and host pieces that the two depth kernels of information.hip
// (sdfr_render_information, sdfr_render_information_shape) share: the tile shape, the view set-up, the tile cull, the
// tile's pixels with the inclusion rule, the per-pixel pose derivatives, the cell of a pixel's latent features and the
// sizes of the flag block.  One statement of each: both kernels include a pixel by the same rule and form its d with
// the same instructions.
#pragma once
#include <climits>

#include "device.hpp"

namespace sdfr {
namespace {

constexpr int kInfoBlock = 256;                         // 4 waves
constexpr int kInfoSubs = 2;                            // 32 x 8 sub-tiles side by side: tiles of 64 x 8 pixels
constexpr int kInfoTileW = kInfoSubs * kSubW, kInfoTileH = kSubH;

// the pose part of a view's record, with the expressions of the renderer's own set-up (render.hip, setup_pose): the
// tile kernel forms it itself, from scalar loads -- one launch, no set-up kernel in front of it
__device__ __forceinline__ void info_pose(int b, const float* __restrict__ pos, const float* __restrict__ quat,
                                          const float* __restrict__ inv_scale, ViewSetup& s) {
  const float x = quat[4 * b], y = quat[4 * b + 1], z = quat[4 * b + 2], w = quat[4 * b + 3];
  const V3 p = mk(pos[3 * b], pos[3 * b + 1], pos[3 * b + 2]);
  const float isc = inv_scale[b];
  s.rot[0] = 1 - 2 * (y * y + z * z); s.rot[1] = 2 * (x * y - w * z);     s.rot[2] = 2 * (x * z + w * y);
  s.rot[3] = 2 * (x * y + w * z);     s.rot[4] = 1 - 2 * (x * x + z * z); s.rot[5] = 2 * (y * z - w * x);
  s.rot[6] = 2 * (x * z - w * y);     s.rot[7] = 2 * (y * z + w * x);     s.rot[8] = 1 - 2 * (x * x + y * y);
  s.e[0] = s.rot[0] * p.x + s.rot[3] * p.y + s.rot[6] * p.z;
  s.e[1] = s.rot[1] * p.x + s.rot[4] * p.y + s.rot[7] * p.z;
  s.e[2] = s.rot[2] * p.x + s.rot[5] * p.y + s.rot[8] * p.z;
  s.p[0] = p.x; s.p[1] = p.y; s.p[2] = p.z;
  s.q[0] = x; s.q[1] = y; s.q[2] = z; s.q[3] = w;
  s.scale = 1.0f / isc;
  s.isc = isc;
}

// Can a tile hold a hit pixel at all?  A hit lies inside the grid's cube, the cube inside its bounding sphere, and the
// sphere (centre p, radius sqrt(3) scale, wholly in front of the camera) projects into the rectangle between its four
// tangent planes through the camera's axes: tan = (X D +- r sqrt(X^2 + D^2 - r^2)) / (D^2 - r^2) with D = -p.z.  Two
// pixels and a share of the focal length of slack, as the renderer's own rectangles have.  Every comparison is written
// so that a NaN or a sphere that reaches the camera keeps the tile.
__device__ __forceinline__ bool info_tile_culled(const ViewSetup& s, int px0, int py0, float cx, float cy, float fx,
                                                 float fy) {
  const float r = 1.7321f * 1.001f * fabsf(s.scale), D = -s.p[2];
  const float den = D * D - r * r;
  if (!(D > r) || !(den > 1e-6f * D * D)) return false;
  const float rx = r * sqrtf(fmaxf(fmaf(s.p[0], s.p[0], den), 0.0f)), ry = r * sqrtf(fmaxf(fmaf(s.p[1], s.p[1], den), 0.0f));
  const float ua = cx + fx * ((s.p[0] * D - rx) / den), ub = cx + fx * ((s.p[0] * D + rx) / den);
  const float va = cy - fy * ((s.p[1] * D - ry) / den), vb = cy - fy * ((s.p[1] * D + ry) / den);
  const float mx = 2.5f + 1e-4f * fabsf(fx), my = 2.5f + 1e-4f * fabsf(fy);   // (pixel c has its centre at c + 0.5)
  return (float)(px0 + kInfoTileW) < fminf(ua, ub) - mx || (float)px0 > fmaxf(ua, ub) + mx ||
         (float)(py0 + kInfoTileH) < fminf(va, vb) - my || (float)py0 > fmaxf(va, vb) + my;
}

// The prologue of a tile kernel (grid: tiles in x, tiles in y, B) over the kernel's own locals: the view's pose and, per
// lane and sub-tile, the estimate, the target and whether the pixel is included.  false: the tile has no included pixel,
// its 0 flag is written and the workgroup leaves (workgroup-uniform).  The view's pose first (scalar loads): three tiles
// out of four lie outside the object and leave without a pixel read.  Then the estimate, and the target of the hit
// pixels only.
__device__ __forceinline__ bool info_tile_begin(const float* __restrict__ depth, const float* __restrict__ target,
                                                const float* __restrict__ pos, const float* __restrict__ quat,
                                                const float* __restrict__ inv_scale, int W, int H, float cx, float cy,
                                                float fx, float fy, float inlier_threshold, unsigned* __restrict__ flag,
                                                ViewSetup& s, int& row, float (&zs)[kInfoSubs], float (&ts)[kInfoSubs],
                                                bool (&inc)[kInfoSubs]) {
  using PB = Patch<kPatchWBwd>;
  const int b = blockIdx.z;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int px0 = blockIdx.x * kInfoTileW, py0 = blockIdx.y * kInfoTileH;
  info_pose(b, pos, quat, inv_scale, s);
  if (info_tile_culled(s, px0, py0, cx, cy, fx, fy)) {   // workgroup-uniform
    if (tid == 0) *flag = 0u;
    return false;
  }
  const float* zimg = depth + (size_t)b * H * W;
  const float* timg = target + (size_t)b * H * W;
  bool any = false;
  row = py0 + PB::oy(wave) + PB::y(lane);
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
    if (tid == 0) *flag = 0u;
    return false;
  }
  return true;
}

// d depth / d (p, q, inv_scale) of one hit pixel: backward_tile's acc[0 .. 7] terms with upstream gradient 1
template <int RT>
__device__ __forceinline__ void pixel_derivatives(const ViewSetup& s, const float* __restrict__ vol, int R, int row,
                                                  int col, float z, float cx, float cy, float rfx, float rfy,
                                                  float (&dd)[8]) {
  const int Rr = RT > 0 ? RT : R;
  const float h = 0.5f * (float)(Rr - 1);
  const float scale = s.scale, isc = s.isc;
  const HitPoint hp = hit_point(s, row, col, z, cx, cy, rfx, rfy, isc, h);
  const V3 d = hp.d, o = hp.o;
  const float t = hp.t;
  Cell c;
  gather_cell<RT>(vol, R, hp.gx, hp.gy, hp.gz, c);   // (the cell is clamped into the grid whatever z holds)
  const float tri = trilerp(c);
  // gradient of the trilinear value w.r.t. the cell coordinate
  const float ax = 1.0f - c.ox, ay = 1.0f - c.oy, az = 1.0f - c.oz;
  const float c00 = fmaf(c.v[4], c.ox, c.v[0] * ax), c01 = fmaf(c.v[5], c.ox, c.v[1] * ax);
  const float c10 = fmaf(c.v[6], c.ox, c.v[2] * ax), c11 = fmaf(c.v[7], c.ox, c.v[3] * ax);
  V3 G;
  G.x = ((c.v[4] - c.v[0]) * ay + (c.v[6] - c.v[2]) * c.oy) * az +
        ((c.v[5] - c.v[1]) * ay + (c.v[7] - c.v[3]) * c.oy) * c.oz;
  G.y = (c10 - c00) * az + (c11 - c01) * c.oz;
  G.z = fmaf(c11, c.oy, c01 * ay) - fmaf(c10, c.oy, c00 * ay);

  const float adz = fabsf(d.z);
  const float f = scale * adz;
  const float sg = isc * h;
  const float kf = f * sg;
  // position: dc/dp_j = -s * R[j][:]
  const V3 RG = rot_f(s, G);
  dd[0] = -(kf * RG.x); dd[1] = -(kf * RG.y); dd[2] = -(kf * RG.z);
  // quaternion: dc/dq_k = s * (d/dq_k[Rhom^T v] - 2 q_k o), v = t d - p
  const V3 v = mk(fmaf(t, d.x, -s.p[0]), fmaf(t, d.y, -s.p[1]), fmaf(t, d.z, -s.p[2]));
  const V3 u = mk(s.q[0], s.q[1], s.q[2]);
  const float w = s.q[3];
  const float udv = dot(u, v);
  const V3 uxv = cross(u, v);
  const float Gv = dot(G, v), Go = dot(G, o), Gu = dot(G, u);
  const V3 vxG = cross(v, G);
  dd[3] = kf * 2.0f * (-u.x * Gv + udv * G.x + v.x * Gu - w * vxG.x - u.x * Go);
  dd[4] = kf * 2.0f * (-u.y * Gv + udv * G.y + v.y * Gu - w * vxG.y - u.y * Go);
  dd[5] = kf * 2.0f * (-u.z * Gv + udv * G.z + v.z * Gu - w * vxG.z - u.z * Go);
  dd[6] = kf * 2.0f * (w * Gv - dot(G, uxv) - w * Go);
  // inverse scale: dc/ds^-1 = o / g, plus the product rule on scale
  dd[7] = f * h * Go - tri * scale * scale * adz;
}

// Where latent_features blends for a hit pixel and with what weight: the cell is gather_cell's (the same clamped floor of
// the same hit point, no corner read), weight = scale |d.z| -- times a corner's trilinear weight it is d depth / d (that
// corner).  A restatement of what pixel_derivatives has just formed, on purpose: with that function handing its Cell
// and weight back, the compiler contracted its products differently in the kernel for a run-time R, and the matrices
// lost their bits (measured); as it stands the second hit_point folds into the first.
template <int RT>
__device__ __forceinline__ void info_latent_cell(const ViewSetup& s, int R, int row, int col, float z, float cx, float cy,
                                                 float rfx, float rfy, Cell& c, float& weight) {
  const int Rr = RT > 0 ? RT : R;
  const float h = 0.5f * (float)(Rr - 1);
  const HitPoint hp = hit_point(s, row, col, z, cx, cy, rfx, rfy, s.isc, h);
  const float top = (float)(Rr - 2);
  const float bx = fminf(fmaxf(floorf(hp.gx), 0.0f), top);
  const float by = fminf(fmaxf(floorf(hp.gy), 0.0f), top);
  const float bz = fminf(fmaxf(floorf(hp.gz), 0.0f), top);
  c.ox = hp.gx - bx; c.oy = hp.gy - by; c.oz = hp.gz - bz;
  c.lin = (Rr <= 256) ? (int)fmaf(fmaf(bx, (float)Rr, by), (float)Rr, bz) : ((int)bx * Rr + (int)by) * Rr + (int)bz;
  weight = s.scale * fabsf(hp.d.z);
}

inline int info_tiles_x(int W) { return (W + kInfoTileW - 1) / kInfoTileW; }
inline int info_tiles_y(int H) { return (H + kInfoTileH - 1) / kInfoTileH; }
inline bool info_sizes_ok(int B, int W, int H) {
  return B >= 1 && B <= 65535 && W >= 1 && H >= 1 && info_tiles_y(H) <= 65535 && (long long)W * H <= INT_MAX;
}
inline size_t info_flag_bytes(int B, int W, int H) {
  return (((size_t)B * info_tiles_x(W) * info_tiles_y(H) * sizeof(unsigned)) + 127) & ~(size_t)127;
}

}  // namespace
}  // namespace sdfr
