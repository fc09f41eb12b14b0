// mesh_grid.hpp -- how the marching-cubes kernels (mesh.hip) and the bounds reduction (boxes.hip) read a grid and
// where they place the vertex of a crossed edge: one statement of the arithmetic, so that the bounds of a grid are
// bitwise the minimum and maximum of the vertices emitted for it.
#pragma once

#include "common.hpp"

namespace sdfr {

struct MeshGrid {
  const float* sdf;   // grid n's volume: sdf + n R^3
  int R, M, pad;      // pad = 1: the complete mesh's virtual border (M = R + 2)
  float level;
};

// value at padded coordinates (i, j, k) of grid `g`; 1.0 on the virtual border
__device__ __forceinline__ float mesh_at(const float* __restrict__ g, const MeshGrid& p, int i, int j, int k) {
  if (p.pad) {
    i -= 1, j -= 1, k -= 1;
    if ((unsigned)i >= (unsigned)p.R || (unsigned)j >= (unsigned)p.R || (unsigned)k >= (unsigned)p.R) return 1.0f;
  }
  return g[((size_t)i * p.R + j) * p.R + k];
}

// the crossed owned edges of point (i, j, k): bit a = edge along axis a
__device__ __forceinline__ unsigned mesh_owned_edges(const float* __restrict__ g, const MeshGrid& p, int i, int j,
                                                     int k, float v0) {
  const bool in0 = v0 < p.level;
  unsigned m = 0;
  if (i + 1 < p.M && (mesh_at(g, p, i + 1, j, k) < p.level) != in0) m |= 1u;
  if (j + 1 < p.M && (mesh_at(g, p, i, j + 1, k) < p.level) != in0) m |= 2u;
  if (k + 1 < p.M && (mesh_at(g, p, i, j, k + 1) < p.level) != in0) m |= 4u;
  return m;
}

// where the level lies on a crossed edge whose ends have the values v0 (the owner point) and v1: 0 at v0, 1 at v1
__device__ __forceinline__ float mesh_edge_t(float v0, float v1, float level) { return (level - v0) / (v1 - v0); }

// the vertex at t on the edge from point (i, j, k) along axis a
__device__ __forceinline__ V3 mesh_edge_vertex(int i, int j, int k, int a, float t, float s, float h) {
  // (idx - (M - 1) / 2) is exact; t is added once, then scaled once
  float x = (float)i - h, y = (float)j - h, z = (float)k - h;
  if (a == 0) x += t;
  if (a == 1) y += t;
  if (a == 2) z += t;
  return mk(x * s, y * s, z * s);
}

inline int mesh_side(int R, int complete) { return complete ? R + 2 : R; }
// index units -> the reference's frame: idx s - s (M - 1) / 2, s = 2 / (R - 1) (simple_setup.py:647-658)
inline float mesh_vertex_scale(int R) { return 2.0f / (float)(R - 1); }
inline float mesh_vertex_half(int M) { return (float)(M - 1) * 0.5f; }

}  // namespace sdfr
