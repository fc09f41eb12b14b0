// mesh.hip -- marching cubes over N grids (SDFPipeline.generate_mesh, simple_setup.py:621-669), gfx950.
//
// A grid is the decoder's volume sdf[i][j][k] (side R), or with `complete` the same volume inside a virtual border of
// 1.0 (the reference's F.pad(..., value=1.0)): side M = R + 2, read through mesh_at() -- no padded copy.  Grid point
// g = (i M + j) M + k owns the edges g -> g + e_a along the axes a = 0, 1, 2 (e_0 = M^2, e_1 = M, e_2 = 1) and, for
// i, j, k < M - 1, the cell whose minimum corner it is.  A corner is inside iff v < level, an edge is crossed iff its
// ends differ, and every crossed edge carries ONE vertex, shared by the triangles around it.
//
// Ordering contract (what the CPU twin tests/mesh_twin.py reproduces exactly):
//   vertices  by owner point g ascending, then axis 0, 1, 2
//   faces     by cell (its minimum corner g) ascending, then the case table's triangle order (mesh_tables.hpp)
// Both orders are exclusive scans of per-point counts, taken over integers: the output is the same bits every run.
//
// Launch sequence (no workgroup waits on another of the same launch):
//   1. mesh_classify_kernel  (M^3 / 256, N) -- per point: crossed owned edges, the cell's triangle count, the value;
//                            per workgroup: {V, F, min, max} partials
//   2. mesh_scan_kernel      (N)            -- exclusive scan of the partials in place; per grid {V, F, min, max}
//   -- the caller reads the N totals back and allocates exact-size outputs --
//   3. mesh_vertices_kernel  (M^3 / 256, N) -- in-workgroup scan + the workgroup's offset: positions (and normals);
//                            every point's vertex base (| its crossed-edge bits << 29) into the workspace
//   4. mesh_faces_kernel     (M^3 / 256, N) -- in-workgroup scan: the cell's triangles as owner base + edge rank
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "mesh_grid.hpp"
#include "mesh_tables.hpp"

namespace sdfr {
namespace {

constexpr int kMeshThreads = 256;
constexpr int kMeshScanThreads = 1024;
constexpr unsigned kMeshBaseBits = 29;   // vertex base | crossed-edge bits << 29: bases stay below 3 * 258^3 < 2^26
constexpr unsigned kMeshBaseMask = (1u << kMeshBaseBits) - 1u;

// the case tables in the constant address space (read with divergent case indices)
__constant__ unsigned char c_tri_count[256] = {
#define SDFR_X(n) mesh::kTriCount[n]
#define SDFR_X4(n) SDFR_X(n), SDFR_X(n + 1), SDFR_X(n + 2), SDFR_X(n + 3)
#define SDFR_X16(n) SDFR_X4(n), SDFR_X4(n + 4), SDFR_X4(n + 8), SDFR_X4(n + 12)
#define SDFR_X64(n) SDFR_X16(n), SDFR_X16(n + 16), SDFR_X16(n + 32), SDFR_X16(n + 48)
    SDFR_X64(0), SDFR_X64(64), SDFR_X64(128), SDFR_X64(192)};
#undef SDFR_X
#define SDFR_X(n) mesh::kTriTable[(n) >> 4][(n) & 15]
__constant__ signed char c_tri_table[256 * 16] = {SDFR_X64(0), SDFR_X64(64), SDFR_X64(128), SDFR_X64(192),
                                                  SDFR_X64(256), SDFR_X64(320), SDFR_X64(384), SDFR_X64(448),
                                                  SDFR_X64(512), SDFR_X64(576), SDFR_X64(640), SDFR_X64(704),
                                                  SDFR_X64(768), SDFR_X64(832), SDFR_X64(896), SDFR_X64(960),
                                                  SDFR_X64(1024), SDFR_X64(1088), SDFR_X64(1152), SDFR_X64(1216),
                                                  SDFR_X64(1280), SDFR_X64(1344), SDFR_X64(1408), SDFR_X64(1472),
                                                  SDFR_X64(1536), SDFR_X64(1600), SDFR_X64(1664), SDFR_X64(1728),
                                                  SDFR_X64(1792), SDFR_X64(1856), SDFR_X64(1920), SDFR_X64(1984),
                                                  SDFR_X64(2048), SDFR_X64(2112), SDFR_X64(2176), SDFR_X64(2240),
                                                  SDFR_X64(2304), SDFR_X64(2368), SDFR_X64(2432), SDFR_X64(2496),
                                                  SDFR_X64(2560), SDFR_X64(2624), SDFR_X64(2688), SDFR_X64(2752),
                                                  SDFR_X64(2816), SDFR_X64(2880), SDFR_X64(2944), SDFR_X64(3008),
                                                  SDFR_X64(3072), SDFR_X64(3136), SDFR_X64(3200), SDFR_X64(3264),
                                                  SDFR_X64(3328), SDFR_X64(3392), SDFR_X64(3456), SDFR_X64(3520),
                                                  SDFR_X64(3584), SDFR_X64(3648), SDFR_X64(3712), SDFR_X64(3776),
                                                  SDFR_X64(3840), SDFR_X64(3904), SDFR_X64(3968), SDFR_X64(4032)};
#undef SDFR_X
#undef SDFR_X4
#undef SDFR_X16
#undef SDFR_X64

// the case index of the cell with minimum corner (i, j, k) (all < M - 1)
__device__ __forceinline__ unsigned mesh_cell_case(const float* __restrict__ g, const MeshGrid& p, int i, int j,
                                                   int k) {
  unsigned c = 0;
#pragma unroll
  for (int n = 0; n < 8; ++n)
    c |= (mesh_at(g, p, i + (n & 1), j + ((n >> 1) & 1), k + ((n >> 2) & 1)) < p.level ? 1u : 0u) << n;
  return c;
}

__device__ __forceinline__ int wave_inclusive_scan(int x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

// exclusive scan of two ints over the workgroup (blockDim.x = kThreads); returns the workgroup totals
template <int kThreads>
__device__ __forceinline__ int2 block_exclusive_scan2(int a, int b, int& ea, int& eb) {
  constexpr int kWaves = kThreads / 64;
  __shared__ int s_a[kWaves], s_b[kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ia = wave_inclusive_scan(a), ib = wave_inclusive_scan(b);
  if (lane == 63) s_a[wave] = ia, s_b[wave] = ib;
  __syncthreads();
  int oa = 0, ob = 0, ta = 0, tb = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) oa += s_a[w], ob += s_b[w];
    ta += s_a[w], tb += s_b[w];
  }
  __syncthreads();   // s_a / s_b are reused by the caller's next scan
  ea = oa + ia - a;
  eb = ob + ib - b;
  return make_int2(ta, tb);
}

// sum over grids m < n of totals[m][field] (the grid's first output row), by the whole workgroup
__device__ __forceinline__ long long grid_offset(const int* __restrict__ totals, int n, int field) {
  __shared__ long long s_part[kMeshThreads / 64];
  long long s = 0;
  for (int m = threadIdx.x; m < n; m += kMeshThreads) s += totals[4 * m + field];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
  __syncthreads();
  long long t = 0;
#pragma unroll
  for (int w = 0; w < kMeshThreads / 64; ++w) t += s_part[w];
  __syncthreads();
  return t;
}

__global__ void __launch_bounds__(kMeshThreads) mesh_classify_kernel(MeshGrid p, int4* __restrict__ partials,
                                                                      int nblk) {
  const int n = blockIdx.y;
  const float* __restrict__ g = p.sdf + (size_t)n * p.R * p.R * p.R;
  const int M = p.M;
  const long long pts = (long long)M * M * M;
  const long long pt = (long long)blockIdx.x * kMeshThreads + threadIdx.x;
  int nv = 0, nf = 0;
  float lo = INFINITY, hi = -INFINITY;
  if (pt < pts) {
    const int i = (int)pt / (M * M), j = (int)pt / M % M, k = (int)pt % M;
    const float v0 = mesh_at(g, p, i, j, k);
    lo = hi = v0;
    nv = __popc(mesh_owned_edges(g, p, i, j, k, v0));
    if (i < M - 1 && j < M - 1 && k < M - 1) nf = c_tri_count[mesh_cell_case(g, p, i, j, k)];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    nv += __shfl_xor(nv, d, 64);
    nf += __shfl_xor(nf, d, 64);
    lo = fminf(lo, __shfl_xor(lo, d, 64));
    hi = fmaxf(hi, __shfl_xor(hi, d, 64));
  }
  __shared__ int4 s_w[kMeshThreads / 64];
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = make_int4(nv, nf, __float_as_int(lo), __float_as_int(hi));
  __syncthreads();
  if (threadIdx.x == 0) {
    int4 r = s_w[0];
    for (int w = 1; w < kMeshThreads / 64; ++w) {
      r.x += s_w[w].x, r.y += s_w[w].y;
      r.z = __float_as_int(fminf(__int_as_float(r.z), __int_as_float(s_w[w].z)));
      r.w = __float_as_int(fmaxf(__int_as_float(r.w), __int_as_float(s_w[w].w)));
    }
    partials[(size_t)n * nblk + blockIdx.x] = r;
  }
}

// one workgroup per grid: partials[n][b].{x, y} := the exclusive prefix of the block counts; totals[n] = {V, F, min,
// max} (min / max as float bits)
__global__ void __launch_bounds__(kMeshScanThreads) mesh_scan_kernel(int4* __restrict__ partials, int nblk,
                                                                      int* __restrict__ totals) {
  const int n = blockIdx.x;
  int4* __restrict__ part = partials + (size_t)n * nblk;
  int cv = 0, cf = 0;
  float lo = INFINITY, hi = -INFINITY;
  for (int base = 0; base < nblk; base += kMeshScanThreads) {
    const int b = base + threadIdx.x;
    int4 r = b < nblk ? part[b] : make_int4(0, 0, __float_as_int(INFINITY), __float_as_int(-INFINITY));
    lo = fminf(lo, __int_as_float(r.z));
    hi = fmaxf(hi, __int_as_float(r.w));
    int ev, ef;
    const int2 t = block_exclusive_scan2<kMeshScanThreads>(r.x, r.y, ev, ef);
    if (b < nblk) part[b] = make_int4(cv + ev, cf + ef, r.z, r.w);
    cv += t.x, cf += t.y;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, d, 64));
    hi = fmaxf(hi, __shfl_xor(hi, d, 64));
  }
  __shared__ float s_lo[kMeshScanThreads / 64], s_hi[kMeshScanThreads / 64];
  if ((threadIdx.x & 63) == 0) s_lo[threadIdx.x >> 6] = lo, s_hi[threadIdx.x >> 6] = hi;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kMeshScanThreads / 64; ++w) lo = fminf(lo, s_lo[w]), hi = fmaxf(hi, s_hi[w]);
    totals[4 * n + 0] = cv;
    totals[4 * n + 1] = cf;
    totals[4 * n + 2] = __float_as_int(lo);
    totals[4 * n + 3] = __float_as_int(hi);
  }
}

// np.gradient (edge_order 1) of the padded volume at (i, j, k), index units
__device__ __forceinline__ V3 mesh_gradient(const float* __restrict__ g, const MeshGrid& p, int i, int j, int k) {
  const int M = p.M;
  auto d = [&](int a) {
    const int c = a == 0 ? i : (a == 1 ? j : k);
    const int di = a == 0, dj = a == 1, dk = a == 2;
    if (c == 0) return mesh_at(g, p, i + di, j + dj, k + dk) - mesh_at(g, p, i, j, k);
    if (c == M - 1) return mesh_at(g, p, i, j, k) - mesh_at(g, p, i - di, j - dj, k - dk);
    return 0.5f * (mesh_at(g, p, i + di, j + dj, k + dk) - mesh_at(g, p, i - di, j - dj, k - dk));
  };
  return mk(d(0), d(1), d(2));
}

__global__ void __launch_bounds__(kMeshThreads) mesh_vertices_kernel(MeshGrid p, const int4* __restrict__ partials,
                                                                      int nblk, const int* __restrict__ totals,
                                                                      unsigned* __restrict__ vbase, float s, float h,
                                                                      float* __restrict__ vertices,
                                                                      float* __restrict__ normals) {
  const int n = blockIdx.y;
  const float* __restrict__ g = p.sdf + (size_t)n * p.R * p.R * p.R;
  const int M = p.M;
  const long long pts = (long long)M * M * M;
  const long long pt = (long long)blockIdx.x * kMeshThreads + threadIdx.x;
  const long long row0 = grid_offset(totals, n, 0);
  int i = 0, j = 0, k = 0;
  unsigned m = 0;
  float v0 = 0.0f;
  if (pt < pts) {
    i = (int)pt / (M * M), j = (int)pt / M % M, k = (int)pt % M;
    v0 = mesh_at(g, p, i, j, k);
    m = mesh_owned_edges(g, p, i, j, k, v0);
  }
  int ev, unused;
  block_exclusive_scan2<kMeshThreads>(__popc(m), 0, ev, unused);
  if (pt >= pts) return;
  const unsigned base = (unsigned)(partials[(size_t)n * nblk + blockIdx.x].x + ev);
  vbase[(size_t)n * pts + pt] = base | (m << kMeshBaseBits);
  if (!m) return;
  const V3 ga = normals ? mesh_gradient(g, p, i, j, k) : mk(0.f, 0.f, 0.f);
  long long row = row0 + base;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(m & (1u << a))) continue;
    const int di = a == 0, dj = a == 1, dk = a == 2;
    const float v1 = mesh_at(g, p, i + di, j + dj, k + dk);
    const float t = mesh_edge_t(v0, v1, p.level);
    const V3 pos = mesh_edge_vertex(i, j, k, a, t, s, h);
    float* vo = vertices + 3 * row;
    vo[0] = pos.x;
    vo[1] = pos.y;
    vo[2] = pos.z;
    if (normals) {
      const V3 gb = mesh_gradient(g, p, i + di, j + dj, k + dk);
      const V3 gn = ga + t * (gb - ga);
      const float len = sqrtf(gn.x * gn.x + gn.y * gn.y + gn.z * gn.z);
      const float inv = len > 0.0f ? 1.0f / len : 0.0f;
      float* no = normals + 3 * row;
      no[0] = gn.x * inv;
      no[1] = gn.y * inv;
      no[2] = gn.z * inv;
    }
    ++row;
  }
}

__global__ void __launch_bounds__(kMeshThreads) mesh_faces_kernel(MeshGrid p, const int4* __restrict__ partials,
                                                                   int nblk, const int* __restrict__ totals,
                                                                   const unsigned* __restrict__ vbase,
                                                                   int* __restrict__ faces) {
  const int n = blockIdx.y;
  const float* __restrict__ g = p.sdf + (size_t)n * p.R * p.R * p.R;
  const int M = p.M;
  const long long pts = (long long)M * M * M;
  const long long pt = (long long)blockIdx.x * kMeshThreads + threadIdx.x;
  const long long row0 = grid_offset(totals, n, 1);
  unsigned cs = 0;
  int nt = 0;
  if (pt < pts) {
    const int i = (int)pt / (M * M), j = (int)pt / M % M, k = (int)pt % M;
    if (i < M - 1 && j < M - 1 && k < M - 1) {
      cs = mesh_cell_case(g, p, i, j, k);
      nt = c_tri_count[cs];
    }
  }
  int ef, unused;
  block_exclusive_scan2<kMeshThreads>(nt, 0, ef, unused);
  if (!nt) return;
  const unsigned* __restrict__ vb = vbase + (size_t)n * pts;
  int* fo = faces + 3 * (row0 + partials[(size_t)n * nblk + blockIdx.x].y + ef);
  const signed char* tri = c_tri_table + 16 * cs;
  for (int q = 0; q < 3 * nt; ++q) {
    const int e = tri[q];
    const int c0 = mesh::kEdgeCorner0[e], a = e >> 2;   // edge e = 4 a + ...
    const long long owner = pt + (long long)(c0 & 1) * M * M + ((c0 >> 1) & 1) * M + ((c0 >> 2) & 1);
    const unsigned w = vb[owner];
    fo[q] = (int)((w & kMeshBaseMask) + __popc((w >> kMeshBaseBits) & ((1u << a) - 1u)));
  }
}

inline int mesh_check(const char* fn, int N, int R, int complete) {
  if (N < 1) return fail(SDFR_E_INVALID, "%s: N=%d must be >= 1", fn, N);
  if (N > 65535) return fail(SDFR_E_INVALID, "%s: N=%d exceeds 65535 grids per call", fn, N);
  if (R < 2 || R > 256) return fail(SDFR_E_INVALID, "%s: R=%d out of range [2,256]", fn, R);
  if (complete != 0 && complete != 1) return fail(SDFR_E_INVALID, "%s: complete=%d must be 0 or 1", fn, complete);
  return 0;
}

inline int mesh_blocks(int M) { return (int)(((long long)M * M * M + kMeshThreads - 1) / kMeshThreads); }
inline size_t mesh_partials_bytes(int N, int M) { return (size_t)N * mesh_blocks(M) * sizeof(int4); }

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" int sdfr_mesh_tables(unsigned short* h_edge_mask, signed char* h_tri_table) {
  if (!h_edge_mask || !h_tri_table) return fail(SDFR_E_NULL, "sdfr_mesh_tables: NULL pointer argument");
  for (int c = 0; c < 256; ++c) {
    h_edge_mask[c] = mesh::kEdgeMask[c];
    for (int q = 0; q < 16; ++q) h_tri_table[16 * c + q] = mesh::kTriTable[c][q];
  }
  return 0;
}

extern "C" size_t sdfr_mesh_workspace_bytes(int N, int R, int complete) {
  if (mesh_check("sdfr_mesh_workspace_bytes", N, R, complete)) return 0;
  const int M = mesh_side(R, complete);
  return mesh_partials_bytes(N, M) + (size_t)N * M * M * M * sizeof(unsigned);
}

extern "C" int sdfr_mesh_count(const float* sdf, int N, int R, int complete, float level, int* totals,
                               void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (int rc = mesh_check("sdfr_mesh_count", N, R, complete)) return rc;
  if (!sdf || !totals || !workspace) return fail(SDFR_E_NULL, "sdfr_mesh_count: NULL pointer argument");
  const size_t need = sdfr_mesh_workspace_bytes(N, R, complete);
  if (workspace_bytes < need)
    return fail(SDFR_E_WORKSPACE, "sdfr_mesh_count: workspace %zu < %zu bytes", workspace_bytes, need);
  SDFR_HIP_TRY(hipSetDevice(device));
  const int M = mesh_side(R, complete), nblk = mesh_blocks(M);
  const MeshGrid p{sdf, R, M, complete, level};
  int4* partials = (int4*)workspace;
  hipLaunchKernelGGL(mesh_classify_kernel, dim3(nblk, N), dim3(kMeshThreads), 0, (hipStream_t)stream, p, partials,
                     nblk);
  hipLaunchKernelGGL(mesh_scan_kernel, dim3(N), dim3(kMeshScanThreads), 0, (hipStream_t)stream, partials, nblk,
                     totals);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_mesh_emit(const float* sdf, int N, int R, int complete, float level, const int* totals,
                              float* vertices, float* normals, int* faces, void* workspace, size_t workspace_bytes,
                              int device, void* stream) {
  if (int rc = mesh_check("sdfr_mesh_emit", N, R, complete)) return rc;
  if (!sdf || !totals || !vertices || !faces || !workspace)
    return fail(SDFR_E_NULL, "sdfr_mesh_emit: NULL pointer argument (only normals may be NULL)");
  const size_t need = sdfr_mesh_workspace_bytes(N, R, complete);
  if (workspace_bytes < need)
    return fail(SDFR_E_WORKSPACE, "sdfr_mesh_emit: workspace %zu < %zu bytes", workspace_bytes, need);
  SDFR_HIP_TRY(hipSetDevice(device));
  const int M = mesh_side(R, complete), nblk = mesh_blocks(M);
  const MeshGrid p{sdf, R, M, complete, level};
  const int4* partials = (const int4*)workspace;
  unsigned* vbase = (unsigned*)((char*)workspace + mesh_partials_bytes(N, M));
  const float s = mesh_vertex_scale(R), h = mesh_vertex_half(M);
  hipLaunchKernelGGL(mesh_vertices_kernel, dim3(nblk, N), dim3(kMeshThreads), 0, (hipStream_t)stream, p, partials,
                     nblk, totals, vbase, s, h, vertices, normals);
  hipLaunchKernelGGL(mesh_faces_kernel, dim3(nblk, N), dim3(kMeshThreads), 0, (hipStream_t)stream, p, partials, nblk,
                     totals, (const unsigned*)vbase, faces);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
