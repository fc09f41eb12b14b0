// raster.hip -- depth images of triangle meshes (sdfr_mesh_depth), gfx950.
//
// What the reference does with an off-screen Open3D window (estimation/synthetic.py::draw_depth_geometry): the z-depth
// of the nearest triangle along every pixel-centre ray, 0 where the ray meets none.  K images per call, image k from
// record k of the sdfr_sample_mesh table (K poses of one mesh and K different meshes are the same call).
//
// Launch sequence (no global float atomics, no allocation, no host synchronisation):
//   1. raster_rect_init_kernel (1)               -- rect[k] := empty
//   2. raster_rect_kernel  (F_max / 1024, K)     -- every lane poses four triangles; the union of their conservative
//                                                   pixel bounds goes through a wave and an LDS reduction and four
//                                                   integer atomicMin / atomicMax per workgroup into rect[k]
//   3. raster_tile_kernel  (W / 32, H / 8, K)    -- one workgroup of 256 lanes owns a 32 x 8 pixel tile of one image;
//                                                   a tile outside rect[k] stores zeros and leaves; the others stream
//                                                   the image's triangles in chunks of 256: each lane sets one triangle
//                                                   up (gather, index order, pose), tests it against the four planes
//                                                   that bound the tile's rays, and gives the survivors their edge
//                                                   terms; they are compacted into LDS (a ballot per wave); every
//                                                   lane tests its own pixel against the survivors, the minimum in a
//                                                   register; plain stores at the end
// The set-up is recomputed per tile instead of stored per (image, triangle): the workspace is 16 bytes per image.
//
// Edge terms.  With the camera at the origin the ray of a pixel is d = (dx, dy, 1) (internal frame: x right, y down, z
// forward; an OpenGL-frame vertex has its y and z negated first), and the barycentric weight of vertex i is the scalar
// triple product d . (p x q) over the opposite edge p -> q.  It is formed as d . (p x (q - p)) -- equal in exact
// arithmetic, without the cancellation -- from the edge's two vertices in ONE order (lower vertex index first), and
// the edge vector n = p x (q - p) is negated for the triangle that walks the edge the other way: the two triangles of
// a shared edge see exactly opposite values in every pixel (fma(-a, b, -c) = -fma(a, b, c)), so with the inclusive
// test no pixel centre falls between them.  The file is compiled without floating-point contraction; every fused
// operation is an explicit fmaf, so a triangle's numbers do not depend on where its set-up was inlined.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.hpp"
#include "mesh_record.hpp"

#pragma clang fp contract(off)

namespace sdfr {
namespace {

constexpr int kRasterThreads = 256;
constexpr int kTileW = 32;
constexpr int kTileH = 8;
static_assert(kTileW * kTileH == kRasterThreads, "one lane per pixel of the tile");
constexpr int kRectFaces = 4 * kRasterThreads;     // triangles per workgroup of the rectangle kernel

// the record's pose in the internal frame (the camera looks along +z, y down): an OpenGL-frame pose has its y and z
// negated
__device__ __forceinline__ MeshPose raster_pose(const sdfr_sample_mesh& r, int flags) {
  return mesh_pose(r, (flags & SDFR_MESH_DEPTH_OPEN3D) ? 1.0f : -1.0f);
}

// n = p x (q - p) of the edge between vertices a and b (indices ia != ib), walked a -> b by the triangle: from the
// lower index to the higher one, negated when that is not the triangle's direction
__device__ __forceinline__ V3 raster_edge(V3 a, int ia, V3 b, int ib) {
  const bool fwd = ia < ib;
  const V3 p = fwd ? a : b, q = fwd ? b : a;
  const V3 e = mk(q.x - p.x, q.y - p.y, q.z - p.z);
  const V3 n = mk(fmaf(p.y, e.z, -(p.z * e.y)), fmaf(p.z, e.x, -(p.x * e.z)), fmaf(p.x, e.y, -(p.y * e.x)));
  return fwd ? n : mk(-n.x, -n.y, -n.z);
}

// One triangle, set up for rays from the origin: the edge vectors (weight of vertex i = d . n[i], i opposite the
// edge) and the vertex depths
struct RasterTri {
  V3 n0, n1, n2;
  float z0, z1, z2;
};

__device__ __forceinline__ int raster_clamp_int(float v, int lo, int hi) {
  // v may be +-inf; the comparisons come first, the conversion sees a value inside the image only
  return v <= (float)lo ? lo : (v >= (float)hi ? hi : (int)v);
}

// The loads of a triangle: the face's indices in index order, its raw vertices.
struct RasterFetch {
  int ia, ib, ic;
  float a[3], b[3], c[3];
  bool ok;   // the indices are distinct and inside [0, num_vertices): the vertices were read
};

__device__ __forceinline__ RasterFetch raster_fetch(const float* __restrict__ vertices, int num_vertices,
                                                    const int* __restrict__ faces, int t, bool in_range) {
  RasterFetch r;
  r.ok = false;
  if (!in_range) return r;
  // the vertices in index order: every number below depends on the SET of the three indices alone, so triangles over
  // the same three vertices, in whatever order or winding, give bitwise equal depths (both faces count anyway)
  if (mesh_sorted_face(faces, t, num_vertices, r.ia, r.ib, r.ic) == 0.0f) return r;
  const int ia = r.ia, ib = r.ib, ic = r.ic;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    r.a[j] = vertices[3 * (long long)ia + j];
    r.b[j] = vertices[3 * (long long)ib + j];
    r.c[j] = vertices[3 * (long long)ic + j];
  }
  r.ok = true;
  return r;
}

// The posed vertices; false: the triangle covers nothing (an index outside [0, num_vertices), a repeated index, a
// non-finite vertex, zero area, or every vertex at or behind the camera plane)
__device__ __forceinline__ bool raster_posed(const MeshPose& pose, const RasterFetch& r, V3& A, V3& B, V3& C) {
  if (!r.ok) return false;
  A = mesh_posed_vertex(pose, r.a), B = mesh_posed_vertex(pose, r.b), C = mesh_posed_vertex(pose, r.c);
  const float sum = (A.x + A.y + A.z) + (B.x + B.y + B.z) + (C.x + C.y + C.z);
  if (!(fabsf(sum) < INFINITY)) return false;   // a NaN or an infinity somewhere
  if (!(fmaxf(A.z, fmaxf(B.z, C.z)) > 0.0f)) return false;   // a hit has 0 < depth <= the largest vertex depth
  // zero area (two vertices in one place, three on a line where the subtraction shows it): nothing to draw
  const V3 nrm = cross(B - A, C - A);
  return !(nrm.x == 0.0f && nrm.y == 0.0f && nrm.z == 0.0f);
}

__device__ __forceinline__ void raster_edges(V3 A, V3 B, V3 C, const RasterFetch& r, RasterTri& tri) {
  tri.n0 = raster_edge(B, r.ib, C, r.ic);
  tri.n1 = raster_edge(C, r.ic, A, r.ia);
  tri.n2 = raster_edge(A, r.ia, B, r.ib);
  tri.z0 = A.z, tri.z1 = B.z, tri.z2 = C.z;
}

// A conservative pixel bound [x0, x1] x [y0, y1] of a posed triangle (inclusive, clipped to the image; false: empty),
// for the screen rectangle of the whole mesh.  Projection may be used here and only here: a triangle with a vertex at
// or behind the camera plane has an unbounded image and takes the whole screen.
__device__ __forceinline__ bool raster_bound(V3 A, V3 B, V3 C, int W, int H, float cx, float cy, float fx, float fy,
                                             int& x0, int& y0, int& x1, int& y1) {
  if (fminf(A.z, fminf(B.z, C.z)) > 0.0f) {
    // all three in front: the projection's bounding box, widened by a pixel on every side (the float error of a
    // projected coordinate is far below that wherever it lies inside the image)
    const float ua = A.x / A.z, ub = B.x / B.z, uc = C.x / C.z;
    const float va = A.y / A.z, vb = B.y / B.z, vc = C.y / C.z;
    const float u0 = fmaf(fx, fminf(ua, fminf(ub, uc)), cx - 0.5f), u1 = fmaf(fx, fmaxf(ua, fmaxf(ub, uc)), cx - 0.5f);
    const float v0 = fmaf(fy, fminf(va, fminf(vb, vc)), cy - 0.5f), v1 = fmaf(fy, fmaxf(va, fmaxf(vb, vc)), cy - 0.5f);
    x0 = raster_clamp_int(floorf(u0) - 1.0f, 0, W);        // W / H: past the image (an empty range)
    y0 = raster_clamp_int(floorf(v0) - 1.0f, 0, H);
    x1 = raster_clamp_int(ceilf(u1) + 1.0f, -1, W - 1);
    y1 = raster_clamp_int(ceilf(v1) + 1.0f, -1, H - 1);
  } else {
    x0 = 0, y0 = 0, x1 = W - 1, y1 = H - 1;
  }
  return x0 <= x1 && y0 <= y1;
}

// Can the triangle be met by a ray d = (dx, dy, 1) with dx in [ax0, ax1] and dy in [ay0, ay1]?  A hit point t d (t > 0)
// has x - ax0 z = t (dx - ax0) >= 0, and is a convex combination of the vertices: if x - ax0 z < 0 at all three
// vertices there is no hit, wherever the vertices are -- behind the camera included.  Likewise for the other three
// planes.  No projection, no division.
__device__ __forceinline__ bool raster_meets(V3 A, V3 B, V3 C, float ax0, float ay0, float ax1, float ay1) {
  const bool left = fmaf(-ax0, A.z, A.x) < 0.0f && fmaf(-ax0, B.z, B.x) < 0.0f && fmaf(-ax0, C.z, C.x) < 0.0f;
  const bool right = fmaf(-ax1, A.z, A.x) > 0.0f && fmaf(-ax1, B.z, B.x) > 0.0f && fmaf(-ax1, C.z, C.x) > 0.0f;
  const bool above = fmaf(-ay0, A.z, A.y) < 0.0f && fmaf(-ay0, B.z, B.y) < 0.0f && fmaf(-ay0, C.z, C.y) < 0.0f;
  const bool below = fmaf(-ay1, A.z, A.y) > 0.0f && fmaf(-ay1, B.z, B.y) > 0.0f && fmaf(-ay1, C.z, C.y) > 0.0f;
  return !(left || right || above || below);
}

__global__ void raster_rect_init_kernel(int* __restrict__ rect, int K, int W, int H) {
  const int k = blockIdx.x * kRasterThreads + threadIdx.x;
  if (k >= K) return;
  rect[4 * k] = W, rect[4 * k + 1] = H, rect[4 * k + 2] = -1, rect[4 * k + 3] = -1;
}

__global__ void __launch_bounds__(kRasterThreads) raster_rect_kernel(const sdfr_sample_mesh* __restrict__ meshes,
                                                                      int max_faces, int W, int H, float cx, float cy,
                                                                      float fx, float fy, int flags,
                                                                      int* __restrict__ rect) {
  const int k = blockIdx.y;
  const sdfr_sample_mesh rec = meshes[k];
  const int F = mesh_record_faces(rec, max_faces);
  const long long first = (long long)blockIdx.x * kRectFaces;
  if (first >= F) return;   // uniform over the workgroup
  const MeshPose pose = raster_pose(rec, flags);
  int x0 = W, y0 = H, x1 = -1, y1 = -1;
#pragma unroll
  for (int u = 0; u < kRectFaces / kRasterThreads; ++u) {
    const long long t = first + u * kRasterThreads + threadIdx.x;
    const RasterFetch r = raster_fetch(rec.vertices, rec.num_vertices, rec.faces, (int)t, t < F);
    V3 A, B, C;
    int a0, b0, a1, b1;
    if (raster_posed(pose, r, A, B, C) && raster_bound(A, B, C, W, H, cx, cy, fx, fy, a0, b0, a1, b1))
      x0 = min(x0, a0), y0 = min(y0, b0), x1 = max(x1, a1), y1 = max(y1, b1);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    x0 = min(x0, __shfl_xor(x0, d, 64));
    y0 = min(y0, __shfl_xor(y0, d, 64));
    x1 = max(x1, __shfl_xor(x1, d, 64));
    y1 = max(y1, __shfl_xor(y1, d, 64));
  }
  __shared__ int s_box[kRasterThreads / 64][4];
  if ((threadIdx.x & 63) == 0) {
    int* b = s_box[threadIdx.x >> 6];
    b[0] = x0, b[1] = y0, b[2] = x1, b[3] = y1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kRasterThreads / 64; ++w)
      x0 = min(x0, s_box[w][0]), y0 = min(y0, s_box[w][1]), x1 = max(x1, s_box[w][2]), y1 = max(y1, s_box[w][3]);
    if (x0 <= x1 && y0 <= y1) {
      // one set of integer minima and maxima per workgroup: the result does not depend on the order of arrival
      atomicMin(rect + 4 * k, x0);
      atomicMin(rect + 4 * k + 1, y0);
      atomicMax(rect + 4 * k + 2, x1);
      atomicMax(rect + 4 * k + 3, y1);
    }
  }
}

__global__ void __launch_bounds__(kRasterThreads) raster_tile_kernel(const sdfr_sample_mesh* __restrict__ meshes,
                                                                      int max_faces, int W, int H, float cx, float cy,
                                                                      float fx, float fy, float near, int flags,
                                                                      const int* __restrict__ rect,
                                                                      float* __restrict__ depth,
                                                                      int* __restrict__ triangle) {
  const int k = blockIdx.z;
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  const int col = tx0 + (threadIdx.x & (kTileW - 1)), row = ty0 + (threadIdx.x >> 5);
  const bool inside = col < W && row < H;
  const size_t pix = ((size_t)k * H + (inside ? row : 0)) * W + (inside ? col : 0);
  const int tx1 = min(tx0 + kTileW, W) - 1, ty1 = min(ty0 + kTileH, H) - 1;   // the tile, inclusive
  const int rx0 = rect[4 * k], ry0 = rect[4 * k + 1], rx1 = rect[4 * k + 2], ry1 = rect[4 * k + 3];

  float best = INFINITY;
  int best_t = -1;
  const sdfr_sample_mesh rec = meshes[k];
  const int F = mesh_record_faces(rec, max_faces);
  if (F > 0 && rx0 <= tx1 && rx1 >= tx0 && ry0 <= ty1 && ry1 >= ty0) {   // uniform over the workgroup
    const MeshPose pose = raster_pose(rec, flags);
    const float dx = ((float)col + 0.5f - cx) / fx, dy = ((float)row + 0.5f - cy) / fy;
    // the tile's rays, with half a pixel to spare on every side (far more than the rounding of these four numbers and
    // of the tests on them can move a plane)
    const float ax0 = ((float)tx0 - cx) / fx, ax1 = ((float)(tx1 + 1) - cx) / fx;
    const float ay0 = ((float)ty0 - cy) / fy, ay1 = ((float)(ty1 + 1) - cy) / fy;
    __shared__ float4 s_tri[kRasterThreads][4];   // n0 z0 | n1 z1 | n2 z2 | face, -, -, -   (16 KiB)
    __shared__ int s_count[kRasterThreads / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int base = 0; base < F; base += kRasterThreads) {
      const int t = base + threadIdx.x;
      const RasterFetch fetched = raster_fetch(rec.vertices, rec.num_vertices, rec.faces, t, t < F);
      RasterTri tri;
      V3 A, B, C;
      const bool keep = raster_posed(pose, fetched, A, B, C) && raster_meets(A, B, C, ax0, ay0, ax1, ay1);
      if (keep) raster_edges(A, B, C, fetched, tri);
      const unsigned long long mask = __ballot(keep);
      if (lane == 0) s_count[wave] = __popcll(mask);
      __syncthreads();   // the counts are there; the previous round's records are no longer read
      int slot = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
      for (int w = 0; w < kRasterThreads / 64; ++w) {
        const int c = s_count[w];
        slot += w < wave ? c : 0;
        total += c;
      }
      if (keep) {
        s_tri[slot][0] = make_float4(tri.n0.x, tri.n0.y, tri.n0.z, tri.z0);
        s_tri[slot][1] = make_float4(tri.n1.x, tri.n1.y, tri.n1.z, tri.z1);
        s_tri[slot][2] = make_float4(tri.n2.x, tri.n2.y, tri.n2.z, tri.z2);
        s_tri[slot][3] = make_float4(__int_as_float(t), 0.0f, 0.0f, 0.0f);
      }
      __syncthreads();
      for (int j = 0; j < total; ++j) {
        // the same address in every lane: broadcast reads
        const float4 a = s_tri[j][0], b = s_tri[j][1], c = s_tri[j][2];
        const float w0 = fmaf(a.x, dx, fmaf(a.y, dy, a.z));
        const float w1 = fmaf(b.x, dx, fmaf(b.y, dy, b.z));
        const float w2 = fmaf(c.x, dx, fmaf(c.y, dy, c.z));
        // inclusive, both faces; a NaN weight fails both
        const bool in = (w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f) || (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f);
        const float det = w0 + (w1 + w2);   // summed as the numerator is: a triangle of constant depth gives it exactly
        const float z = fmaf(w0, a.w, fmaf(w1, b.w, w2 * c.w)) / det;   // det = 0: NaN or inf, refused below
        const int f = __float_as_int(s_tri[j][3].x);
        const bool better = in && z > near && z < INFINITY && (z < best || (z == best && f < best_t));
        best = better ? z : best;
        best_t = better ? f : best_t;
      }
      // (the next round's first barrier stands between these reads and its writes)
    }
  }
  if (inside) {
    depth[pix] = best_t >= 0 ? best : 0.0f;
    if (triangle) triangle[pix] = best_t;
  }
}

inline int raster_check(const char* fn, int K, long long total_faces, int max_faces, int W, int H) {
  if (int rc = mesh_table_check(fn, K, total_faces, max_faces)) return rc;
  if (W < 1 || H < 1 || W > 16384 || H > 16384)
    return fail(SDFR_E_INVALID, "%s: image size W=%d, H=%d out of range [1,16384]", fn, W, H);
  return 0;
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_mesh_depth_workspace_bytes(int K, long long total_faces, int max_faces, int W, int H) {
  if (raster_check("sdfr_mesh_depth_workspace_bytes", K, total_faces, max_faces, W, H)) return 0;
  return (size_t)K * 4 * sizeof(int);
}

extern "C" int sdfr_mesh_depth(const sdfr_sample_mesh* meshes, int K, long long total_faces, int max_faces, int W,
                               int H, float cx, float cy, float fx, float fy, float near, int flags, float* depth,
                               int* triangle, void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (int rc = raster_check("sdfr_mesh_depth", K, total_faces, max_faces, W, H)) return rc;
  if (!(fx > 0.0f) || !(fy > 0.0f) || !(fx < INFINITY) || !(fy < INFINITY))
    return fail(SDFR_E_INVALID, "sdfr_mesh_depth: fx=%g, fy=%g must be positive and finite", (double)fx, (double)fy);
  if (!(fabsf(cx) < INFINITY) || !(fabsf(cy) < INFINITY))
    return fail(SDFR_E_INVALID, "sdfr_mesh_depth: cx=%g, cy=%g must be finite", (double)cx, (double)cy);
  if (!(near >= 0.0f) || !(near < INFINITY))
    return fail(SDFR_E_INVALID, "sdfr_mesh_depth: near=%g must be >= 0 and finite", (double)near);
  if (flags & ~SDFR_MESH_DEPTH_OPEN3D)
    return fail(SDFR_E_INVALID, "sdfr_mesh_depth: flags=0x%x has unknown bits", (unsigned)flags);
  if (!meshes || !depth || !workspace)
    return fail(SDFR_E_NULL, "sdfr_mesh_depth: NULL pointer argument (only triangle may be NULL)");
  const size_t need = (size_t)K * 4 * sizeof(int);
  if (workspace_bytes < need)
    return fail(SDFR_E_WORKSPACE, "sdfr_mesh_depth: workspace %zu < %zu bytes", workspace_bytes, need);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  int* rect = (int*)workspace;
  hipLaunchKernelGGL(raster_rect_init_kernel, dim3((K + kRasterThreads - 1) / kRasterThreads), dim3(kRasterThreads), 0,
                     st, rect, K, W, H);
  hipLaunchKernelGGL(raster_rect_kernel, dim3((max_faces + kRectFaces - 1) / kRectFaces, K),
                     dim3(kRasterThreads), 0, st, meshes, max_faces, W, H, cx, cy, fx, fy, flags, rect);
  hipLaunchKernelGGL(raster_tile_kernel, dim3((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH, K),
                     dim3(kRasterThreads), 0, st, meshes, max_faces, W, H, cx, cy, fx, fy, near, flags,
                     (const int*)rect, depth, triangle);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
