// mesh_sdf.hip -- signed distance volumes of triangle meshes (sdfr_mesh_sdf), gfx950.
//
// What the reference does with the external mesh_to_sdf package (vae/sdf_utils.py::mesh_to_sdf: 100 depth scans, a
// KD-tree over the scanned points, the sign from visibility), computed exactly instead: for every point of an R^3 grid
// the Euclidean distance to the closest point of the closest triangle (face interior, edge or vertex), signed by the
// generalised winding number.  K grids per call, grid k from record k of the sdfr_sample_mesh table.  Brute force:
// every grid point meets every face.
//
// Launch sequence (no float atomics, no allocation, no host synchronisation):
//   1. mesh_sdf_head_kernel   (1)                 -- head[k] = {first record, faces} of mesh k: an exclusive scan of the
//                                                    records' face counts (a record that may not be read counts 0)
//   2. mesh_sdf_setup_kernel  (F_max / 256, K)    -- every lane poses one face ONCE and stores its 64-byte record: the
//                                                    three posed vertices in index order as a, b - a, c - a, the squared
//                                                    edge terms, the normal (b - a) x (c - a) and the parity of the
//                                                    sort (0: the face is invalid and contributes nothing)
//   3. mesh_sdf_kernel        (R^3 / 256, K)      -- one workgroup of 256 lanes owns 256 consecutive grid points of one
//                                                    mesh; it streams the mesh's records through LDS in rounds of 256
//                                                    and every lane meets each of them at the same LDS address
//                                                    (broadcast reads): the smallest squared distance and its face in
//                                                    registers, the winding sum in an fp64 register; plain stores
// A face's numbers depend on its three posed vertices, taken in index order, and on the grid point alone; the minimum
// is exact and ties go to the lowest face, so the unsigned field and `triangle` do not depend on the order of the
// faces.  The winding sum is ordered: ascending face index, always (the faces are never sliced over workgroups).
// The file is compiled without floating-point contraction; every fused operation is an explicit fmaf.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.hpp"
#include "mesh_record.hpp"

#pragma clang fp contract(off)

namespace sdfr {
namespace {

constexpr int kSdfThreads = 256;   // lanes per workgroup = grid points per brick = face records per LDS round

struct MeshSdfHead {
  long long offset;   // the mesh's first face record in the workspace
  int faces;          // the faces that are read: the record's num_faces, or 0 (then the grid is NaN)
  int pad;
};
static_assert(sizeof(MeshSdfHead) == 16, "MeshSdfHead must stay 16 bytes");

inline size_t mesh_sdf_head_bytes(int K) { return ((size_t)K * sizeof(MeshSdfHead) + 63) & ~(size_t)63; }

// a x b in plain products and differences: common.hpp's `cross` is defined in front of this file's contraction pragma
// and may be fused there; here two equal products must cancel exactly (three points on a line in one coordinate
// pattern have zero area in fp32 too)
__device__ __forceinline__ V3 mesh_sdf_cross(V3 a, V3 b) {
  return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

// one workgroup: head[k] for all K records.  Thread t scans the records [t c, t c + c), c = ceil(K / 256).
__global__ void __launch_bounds__(kSdfThreads) mesh_sdf_head_kernel(const sdfr_sample_mesh* __restrict__ meshes, int K,
                                                                     long long total_faces, int max_faces,
                                                                     MeshSdfHead* __restrict__ head) {
  __shared__ long long s_sum[kSdfThreads];
  const int chunk = (K + kSdfThreads - 1) / kSdfThreads;
  const int lo = min(K, (int)threadIdx.x * chunk), hi = min(K, lo + chunk);
  long long sum = 0;
  for (int k = lo; k < hi; ++k) sum += mesh_record_faces(meshes[k], max_faces);
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long run = 0;
    for (int t = 0; t < kSdfThreads; ++t) {
      const long long s = s_sum[t];
      s_sum[t] = run;
      run += s;
    }
  }
  __syncthreads();
  long long off = s_sum[threadIdx.x];
  for (int k = lo; k < hi; ++k) {
    const int F = mesh_record_faces(meshes[k], max_faces);
    // records that would leave the workspace (the caller's total_faces is too small) are not written or read
    head[k].offset = off;
    head[k].faces = off + F <= total_faces ? F : 0;
    head[k].pad = 0;
    off += F;
  }
}

// The record of one face, four float4:
//   a.xyz, |ab|^2  |  ab.xyz, ab . ac  |  ac.xyz, |ac|^2  |  n.xyz = ab x ac, parity
// with a, b, c the posed vertices in ascending index order, ab = b - a, ac = c - a, and parity = +1 / -1 where that
// order is an even / odd permutation of the face's own (n * parity is then the face's normal (b - a) x (c - a)), 0 for a
// face that contributes nothing: an index outside [0, num_vertices), a repeated index, a non-finite posed vertex, zero
// area.
__global__ void __launch_bounds__(kSdfThreads) mesh_sdf_setup_kernel(const sdfr_sample_mesh* __restrict__ meshes,
                                                                      const MeshSdfHead* __restrict__ head,
                                                                      float4* __restrict__ records) {
  const int k = blockIdx.y;
  const MeshSdfHead h = head[k];
  const int t = blockIdx.x * kSdfThreads + threadIdx.x;
  if (t >= h.faces) return;
  const sdfr_sample_mesh rec = meshes[k];
  float4* out = records + 4 * (h.offset + t);
  int ia, ib, ic;
  const float parity = mesh_sorted_face(rec.faces, t, rec.num_vertices, ia, ib, ic);
  float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0, r3 = r0;
  if (parity != 0.0f) {   // nothing else is read
    const MeshPose pose = mesh_pose(rec, 1.0f);   // the record's own frame
    const V3 a = mesh_posed_vertex(pose, rec.vertices + 3 * (long long)ia);
    const V3 b = mesh_posed_vertex(pose, rec.vertices + 3 * (long long)ib);
    const V3 c = mesh_posed_vertex(pose, rec.vertices + 3 * (long long)ic);
    const float sum = (a.x + a.y + a.z) + (b.x + b.y + b.z) + (c.x + c.y + c.z);
    const V3 ab = b - a, ac = c - a;
    const V3 n = mesh_sdf_cross(ab, ac);
    // (a NaN or an infinity somewhere fails the first test)
    if (fabsf(sum) < INFINITY && !(n.x == 0.0f && n.y == 0.0f && n.z == 0.0f)) {
      r0 = make_float4(a.x, a.y, a.z, dot(ab, ab));
      r1 = make_float4(ab.x, ab.y, ab.z, dot(ab, ac));
      r2 = make_float4(ac.x, ac.y, ac.z, dot(ac, ac));
      r3 = make_float4(n.x, n.y, n.z, parity);
    }
  }
  out[0] = r0, out[1] = r1, out[2] = r2, out[3] = r3;
}

// Squared distance from the point at p = a + ap to the triangle (a, a + ab, a + ac): the closest point by Voronoi
// region (vertex a, b, edge ab, vertex c, edge ac, edge bc, interior -- the first that applies), as barycentric
// numerators over one denominator, one division.
__device__ __forceinline__ float mesh_sdf_dist2(V3 ap, const float4 q0, const float4 q1, const float4 q2) {
  const V3 ab = mk(q1.x, q1.y, q1.z), ac = mk(q2.x, q2.y, q2.z);
  const float d1 = dot(ab, ap), d2 = dot(ac, ap);
  const float d3 = d1 - q0.w, d4 = d2 - q1.w;   // ab . bp, ac . bp
  const float d5 = d1 - q1.w, d6 = d2 - q2.w;   // ab . cp, ac . cp
  const float vc = fmaf(d1, d4, -(d3 * d2));
  const float vb = fmaf(d5, d2, -(d1 * d6));
  const float va = fmaf(d3, d6, -(d5 * d4));
  const float e43 = d4 - d3, e56 = d5 - d6;
  float vn = vb, wn = vc, den = va + (vb + vc);                     // interior
  bool r = va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f;                // edge bc
  vn = r ? e56 : vn, wn = r ? e43 : wn, den = r ? e43 + e56 : den;
  r = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;                       // edge ac
  vn = r ? 0.0f : vn, wn = r ? d2 : wn, den = r ? d2 - d6 : den;
  r = d6 >= 0.0f && d5 <= d6;                                       // vertex c
  vn = r ? 0.0f : vn, wn = r ? 1.0f : wn, den = r ? 1.0f : den;
  r = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;                       // edge ab
  vn = r ? d1 : vn, wn = r ? 0.0f : wn, den = r ? d1 - d3 : den;
  r = d3 >= 0.0f && d4 <= d3;                                       // vertex b
  vn = r ? 1.0f : vn, wn = r ? 0.0f : wn, den = r ? 1.0f : den;
  r = d1 <= 0.0f && d2 <= 0.0f;                                     // vertex a
  vn = r ? 0.0f : vn, wn = r ? 0.0f : wn, den = r ? 1.0f : den;
  const float inv = 1.0f / den;
  const float v = vn * inv, w = wn * inv;
  const V3 d = mk(fmaf(-w, ac.x, fmaf(-v, ab.x, ap.x)), fmaf(-w, ac.y, fmaf(-v, ab.y, ap.y)),
                  fmaf(-w, ac.z, fmaf(-v, ab.z, ap.z)));
  return dot(d, d);   // NaN for a sliver whose denominator vanished in fp32: it then never is the minimum
}

// The solid angle of the triangle seen from the point (van Oosterom and Strackee), A, B, C = the vertices minus the
// point: 2 atan2(A . (B x C), |A||B||C| + (A . B)|C| + (B . C)|A| + (C . A)|B|).  With B = A + ab and C = A + ac the
// triple product is A . (ab x ac) = A . n.
__device__ __forceinline__ float mesh_sdf_solid_angle(V3 ap, const float4 q1, const float4 q2, const float4 q3) {
  const V3 A = mk(-ap.x, -ap.y, -ap.z);
  const V3 B = mk(A.x + q1.x, A.y + q1.y, A.z + q1.z), C = mk(A.x + q2.x, A.y + q2.y, A.z + q2.z);
  const float det = dot(A, mk(q3.x, q3.y, q3.z));
  const float la = sqrtf(dot(A, A)), lb = sqrtf(dot(B, B)), lc = sqrtf(dot(C, C));
  const float den = fmaf(la * lb, lc, fmaf(dot(A, B), lc, fmaf(dot(B, C), la, dot(C, A) * lb)));
  return (2.0f * atan2f(det, den)) * q3.w;
}

template <bool SIGNED>
__global__ void __launch_bounds__(kSdfThreads) mesh_sdf_kernel(const MeshSdfHead* __restrict__ head,
                                                                const float4* __restrict__ records, int R,
                                                                float* __restrict__ sdf, int* __restrict__ triangle,
                                                                float* __restrict__ winding) {
  const int k = blockIdx.y;
  const long long n = (long long)R * R * R;
  const long long idx = (long long)blockIdx.x * kSdfThreads + threadIdx.x;
  const bool inside_grid = idx < n;
  const int i = (int)(inside_grid ? idx : n - 1);
  // sdf[x][y][z]; point i of an axis sits at (2 i - (R - 1)) / (R - 1): the corners at -1 and 1 exactly
  const int ix = i / (R * R), iy = (i / R) % R, iz = i % R;
  const float span = (float)(R - 1);
  const V3 p = mk((float)(2 * ix - (R - 1)) / span, (float)(2 * iy - (R - 1)) / span, (float)(2 * iz - (R - 1)) / span);

  const MeshSdfHead h = head[k];
  const float4* __restrict__ rec = records + 4 * h.offset;
  __shared__ float4 s_rec[kSdfThreads][4];   // 16 KiB
  float best = INFINITY;
  int best_t = -1;
  double omega = 0.0;
  for (int base = 0; base < h.faces; base += kSdfThreads) {   // uniform over the workgroup
    const int t = base + threadIdx.x;
    __syncthreads();   // the previous round's records are no longer read
    if (t < h.faces) {
#pragma unroll
      for (int u = 0; u < 4; ++u) s_rec[threadIdx.x][u] = rec[4 * (long long)t + u];
    }
    __syncthreads();
    const int count = min(kSdfThreads, h.faces - base);
    for (int j = 0; j < count; ++j) {
      // the same address in every lane: broadcast reads
      const float4 q3 = s_rec[j][3];
      if (q3.w != 0.0f) {   // uniform: an invalid face contributes nothing
        const float4 q0 = s_rec[j][0], q1 = s_rec[j][1], q2 = s_rec[j][2];
        const V3 ap = mk(p.x - q0.x, p.y - q0.y, p.z - q0.z);
        const float d2 = mesh_sdf_dist2(ap, q0, q1, q2);
        const bool better = d2 < best;   // ascending faces: a tie stays with the lowest
        best = better ? d2 : best;
        best_t = better ? base + j : best_t;
        if constexpr (SIGNED) omega += (double)mesh_sdf_solid_angle(ap, q1, q2, q3);
      }
    }
  }
  if (inside_grid) {
    const size_t o = (size_t)k * (size_t)n + (size_t)idx;
    const bool found = best_t >= 0;
    const float d = sqrtf(best);
    const double w = omega / (4.0 * 3.14159265358979323846);
    sdf[o] = found ? ((SIGNED && w > 0.5) ? -d : d) : NAN;
    if (triangle) triangle[o] = best_t;
    if (SIGNED && winding) winding[o] = found ? (float)w : NAN;
  }
}

inline int mesh_sdf_check(const char* fn, int K, long long total_faces, int max_faces, int R) {
  if (int rc = mesh_table_check(fn, K, total_faces, max_faces)) return rc;
  if (R < 2 || R > 256) return fail(SDFR_E_INVALID, "%s: R=%d out of range [2,256]", fn, R);
  return 0;
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_mesh_sdf_workspace_bytes(int K, long long total_faces, int max_faces, int R) {
  if (mesh_sdf_check("sdfr_mesh_sdf_workspace_bytes", K, total_faces, max_faces, R)) return 0;
  return mesh_sdf_head_bytes(K) + (size_t)total_faces * 4 * sizeof(float4);
}

extern "C" int sdfr_mesh_sdf(const sdfr_sample_mesh* meshes, int K, long long total_faces, int max_faces, int R,
                             int flags, float* sdf, int* triangle, float* winding, void* workspace,
                             size_t workspace_bytes, int device, void* stream) {
  if (int rc = mesh_sdf_check("sdfr_mesh_sdf", K, total_faces, max_faces, R)) return rc;
  if (flags != SDFR_MESH_SDF_SIGNED && flags != SDFR_MESH_SDF_UNSIGNED)
    return fail(SDFR_E_INVALID, "sdfr_mesh_sdf: flags=0x%x: SDFR_MESH_SDF_SIGNED or _UNSIGNED expected", (unsigned)flags);
  if (flags == SDFR_MESH_SDF_UNSIGNED && winding)
    return fail(SDFR_E_INVALID, "sdfr_mesh_sdf: winding must be NULL with SDFR_MESH_SDF_UNSIGNED (no winding work)");
  if (!meshes || !sdf || !workspace)
    return fail(SDFR_E_NULL, "sdfr_mesh_sdf: NULL pointer argument (only triangle and winding may be NULL)");
  const size_t need = mesh_sdf_head_bytes(K) + (size_t)total_faces * 4 * sizeof(float4);
  if (workspace_bytes < need)
    return fail(SDFR_E_WORKSPACE, "sdfr_mesh_sdf: workspace %zu < %zu bytes", workspace_bytes, need);
  if ((uintptr_t)workspace % 16)
    return fail(SDFR_E_INVALID, "sdfr_mesh_sdf: workspace must be 16-byte aligned");
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  MeshSdfHead* head = (MeshSdfHead*)workspace;
  float4* records = (float4*)((char*)workspace + mesh_sdf_head_bytes(K));
  const long long n = (long long)R * R * R;
  const dim3 bricks((unsigned)((n + kSdfThreads - 1) / kSdfThreads), K);
  hipLaunchKernelGGL(mesh_sdf_head_kernel, dim3(1), dim3(kSdfThreads), 0, st, meshes, K, total_faces, max_faces, head);
  hipLaunchKernelGGL(mesh_sdf_setup_kernel, dim3((max_faces + kSdfThreads - 1) / kSdfThreads, K), dim3(kSdfThreads), 0,
                     st, meshes, (const MeshSdfHead*)head, records);
  if (flags == SDFR_MESH_SDF_UNSIGNED)
    hipLaunchKernelGGL(mesh_sdf_kernel<false>, bricks, dim3(kSdfThreads), 0, st, (const MeshSdfHead*)head,
                       (const float4*)records, R, sdf, triangle, winding);
  else
    hipLaunchKernelGGL(mesh_sdf_kernel<true>, bricks, dim3(kSdfThreads), 0, st, (const MeshSdfHead*)head,
                       (const float4*)records, R, sdf, triangle, winding);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
