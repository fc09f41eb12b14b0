// mesh_record.hpp -- the one device-side reader of the sdfr_sample_mesh record (include/sdfr.h): which of a record's
// faces may be read, its pose as a matrix, a face's indices in index order.  raster.hip, mesh_sdf.hip and metrics.hip
// include it; the Python side writes the table in one place too (mesh._MeshTable).
#pragma once

#include "common.hpp"

// the pose arithmetic must not depend on the including file: no contraction, every fused operation is an explicit fmaf
// (common.hpp's own helpers stay in front of this line)
#pragma clang fp contract(off)

namespace sdfr {

static_assert(sizeof(sdfr_sample_mesh) == 72, "sdfr_sample_mesh layout is part of the ABI");

// the faces of record r that may be read, or 0 (the record then contributes nothing)
__device__ __forceinline__ int mesh_record_faces(const sdfr_sample_mesh& r, int max_faces) {
  const bool ok = r.vertices && r.faces && r.num_vertices >= 1 && r.num_faces >= 1 && r.num_faces <= max_faces;
  return ok ? r.num_faces : 0;
}

// P = M v + t with M = factor * R(quat), uniform over the workgroup.  sign = +1: the record's own frame; -1: rows 1 and
// 2 of M and t negated, the OpenGL camera frame seen from the internal one (the camera looks along +z, y down).
struct MeshPose {
  float m[9];
  float t[3];
};

__device__ __forceinline__ MeshPose mesh_pose(const sdfr_sample_mesh& r, float sign) {
  const float x = r.quat[0], y = r.quat[1], z = r.quat[2], w = r.quat[3];
  const float f = r.factor;
  const float s = sign;
  MeshPose p;
  // the rotation matrix of a quaternion as pipeline.quaternion_apply applies it (v + 2 w (u x v) + 2 u x (u x v))
  p.m[0] = f * (1.0f - 2.0f * (y * y + z * z));
  p.m[1] = f * (2.0f * (x * y - w * z));
  p.m[2] = f * (2.0f * (x * z + w * y));
  p.m[3] = s * f * (2.0f * (x * y + w * z));
  p.m[4] = s * f * (1.0f - 2.0f * (x * x + z * z));
  p.m[5] = s * f * (2.0f * (y * z - w * x));
  p.m[6] = s * f * (2.0f * (x * z - w * y));
  p.m[7] = s * f * (2.0f * (y * z + w * x));
  p.m[8] = s * f * (1.0f - 2.0f * (x * x + y * y));
  p.t[0] = r.position[0];
  p.t[1] = s * r.position[1];
  p.t[2] = s * r.position[2];
  return p;
}

__device__ __forceinline__ V3 mesh_posed_vertex(const MeshPose& p, const float* __restrict__ v) {
  const float x = v[0], y = v[1], z = v[2];
  return mk(fmaf(p.m[0], x, fmaf(p.m[1], y, fmaf(p.m[2], z, p.t[0]))),
            fmaf(p.m[3], x, fmaf(p.m[4], y, fmaf(p.m[5], z, p.t[1]))),
            fmaf(p.m[6], x, fmaf(p.m[7], y, fmaf(p.m[8], z, p.t[2]))));
}

// Face t's vertex indices in ascending order ia <= ib <= ic: what is computed from them depends on the SET of the three
// alone.  Returns the parity of the sort, +1 / -1 for an even / odd permutation of the face's own order, or 0 when an
// index lies outside [0, num_vertices) or is repeated: no vertex of such a face may be read.
__device__ __forceinline__ float mesh_sorted_face(const int* __restrict__ faces, int t, int num_vertices, int& ia,
                                                  int& ib, int& ic) {
  ia = faces[3 * (long long)t], ib = faces[3 * (long long)t + 1], ic = faces[3 * (long long)t + 2];
  float parity = 1.0f;
  if (ia > ib) { const int s = ia; ia = ib; ib = s; parity = -parity; }
  if (ib > ic) { const int s = ib; ib = ic; ic = s; parity = -parity; }
  if (ia > ib) { const int s = ia; ia = ib; ib = s; parity = -parity; }
  const bool ok = ia >= 0 && ic < num_vertices && ia != ib && ib != ic;
  return ok ? parity : 0.0f;
}

// host: the arguments every entry point that takes the table checks first
inline int mesh_table_check(const char* fn, int K, long long total_faces, int max_faces) {
  if (K < 1 || K > 65535) return fail(SDFR_E_INVALID, "%s: K=%d out of range [1,65535]", fn, K);
  if (total_faces < 1) return fail(SDFR_E_INVALID, "%s: total_faces=%lld must be >= 1", fn, total_faces);
  if (max_faces < 1 || max_faces > total_faces)
    return fail(SDFR_E_INVALID, "%s: max_faces=%d out of range [1,total_faces=%lld]", fn, max_faces, total_faces);
  return 0;
}

}  // namespace sdfr
