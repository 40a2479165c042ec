// pm_mesh_body.hpp -- the arithmetic and the per-thread bodies of pm_grid_mesh (include/pm/imaging.h), host-callable and
// free of kernels like pm_cloud_body.hpp, on which it builds: what COUNTS is cloud_point() + cloud_counts(), a vertex is
// stored by cloud_store().  pm_stages.hip uses it through pm_mesh.hpp, a CPU build (tests/cpp/mesh_host_main.cpp, under
// the sanitizers) runs the same bodies.  The definition it is held to BIT FOR BIT is tests/mesh_ref.py.
//
// Every body works on VALUES: the value of a grid item is its disparity where the item counts and +0.0f where it does not
// or lies outside the grid, so "counts" is `> 0` and a cell that reaches over the grid's edge has no triangle by the
// ordinary rule (two of its corners do not count).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_cloud_body.hpp"

namespace pm {

// What the launches of the mesh share: the cloud's arguments (camera, filter, map, stride grid) and the mesh's own.
struct MeshArgs {
  CloudArgs c;
  int sub_rows;
  float max_diff;
  int referenced;  // 1: PM_MESH_VERTICES_REFERENCED, 0: PM_MESH_VERTICES_ALL
};

// The value of grid item (xs, ys): d where pm_point_cloud counts the pixel, else 0 (outside the grid included).
__host__ __device__ __forceinline__ float mesh_value(const MeshArgs& a, int xs, int ys) {
  if (xs < 0 || ys < 0 || xs >= a.c.sub_cols || ys >= a.sub_rows) return 0.f;
  const int x = xs * a.c.filter.stride, y = ys * a.c.filter.stride;
  const float d = a.c.disp[(size_t)y * a.c.cols + x];
  if (a.c.filter.max_range == 0.f) return cloud_counts(a.c.filter, d > 0.f, d, 0.f) ? d : 0.f;  // no limit: Z is not read
  float p[3];
  const bool ok = cloud_point(a.c.cam, d, x, y, p);
  return cloud_counts(a.c.filter, ok, d, p[2]) ? d : 0.f;
}

// pm_filter_speckles' edge rule between two values; false for a NaN difference.
__host__ __device__ __forceinline__ bool mesh_edge(float p, float q, float max_diff) {
  return p > 0.f && q > 0.f && __builtin_fabs((double)p - (double)q) <= (double)max_diff;
}

constexpr unsigned kMeshT0 = 1u, kMeshT1 = 2u, kMeshDiag1 = 4u;

// The cell with corner values v00 (xs, ys), v10 (xs + 1, ys), v01 (xs, ys + 1), v11 (xs + 1, ys + 1): which of its two
// triangles are emitted (kMeshT0, kMeshT1) and on which diagonal (kMeshDiag1: 10-01, else 00-11).
__host__ __device__ __forceinline__ unsigned mesh_cell(float v00, float v10, float v01, float v11, float max_diff) {
  const bool c00 = v00 > 0.f, c10 = v10 > 0.f, c01 = v01 > 0.f, c11 = v11 > 0.f;
  const int n = (int)c00 + (int)c10 + (int)c01 + (int)c11;
  if (n < 3) return 0u;
  const bool diag1 = n == 4 ? __builtin_fabs((double)v10 - (double)v01) < __builtin_fabs((double)v00 - (double)v11) : !c00 || !c11;
  const bool left = mesh_edge(v00, v01, max_diff), top = mesh_edge(v00, v10, max_diff);
  const bool bottom = mesh_edge(v01, v11, max_diff), right = mesh_edge(v10, v11, max_diff);
  bool t0, t1;
  if (diag1) {
    const bool d = mesh_edge(v10, v01, max_diff);
    t0 = left && d && top;      // (00, 01, 10)
    t1 = d && bottom && right;  // (10, 01, 11)
  } else {
    const bool d = mesh_edge(v00, v11, max_diff);
    t0 = left && bottom && d;  // (00, 01, 11)
    t1 = d && right && top;    // (00, 11, 10)
  }
  return (t0 ? kMeshT0 : 0u) | (t1 ? kMeshT1 : 0u) | (diag1 ? kMeshDiag1 : 0u);
}

// Whether the item in the middle of the 3x3 values v[dy + 1][dx + 1] is a corner of an emitted triangle: it is corner 11
// of the cell up-left, 01 of the cell above, 10 of the cell to the left and 00 of its own.  Diagonal 0 joins 00 and 11,
// so those two are in both triangles and 10 / 01 in one each; diagonal 1 the other way round.  An emitted triangle's
// corners all count, so no test of the item itself is needed.  mesh_referenced_cells: from mesh_cell()'s values of those
// four cells (the kernels share them between neighbours through LDS); mesh_referenced: from the values.
__host__ __device__ __forceinline__ bool mesh_referenced_cells(unsigned ul, unsigned up, unsigned lf, unsigned own) {
  const unsigned both = kMeshT0 | kMeshT1;
  const bool as11 = (ul & kMeshDiag1) ? (ul & kMeshT1) != 0 : (ul & both) != 0;
  const bool as01 = (up & kMeshDiag1) ? (up & both) != 0 : (up & kMeshT0) != 0;
  const bool as10 = (lf & kMeshDiag1) ? (lf & both) != 0 : (lf & kMeshT1) != 0;
  const bool as00 = (own & kMeshDiag1) ? (own & kMeshT0) != 0 : (own & both) != 0;
  return as11 || as01 || as10 || as00;
}
__host__ __device__ __forceinline__ bool mesh_referenced(const float v[3][3], float max_diff) {
  return mesh_referenced_cells(mesh_cell(v[0][0], v[0][1], v[1][0], v[1][1], max_diff),   // the item is its 11
                               mesh_cell(v[0][1], v[0][2], v[1][1], v[1][2], max_diff),   // ... its 01
                               mesh_cell(v[1][0], v[1][1], v[2][0], v[2][1], max_diff),   // ... its 10
                               mesh_cell(v[1][1], v[1][2], v[2][1], v[2][2], max_diff));  // ... its 00
}

// The vertex of grid item (xs, ys) into slot `slot`: the organised slot map always (the untruncated numbering, -1 where
// the item is no vertex), the streams -- pm_point_cloud's bytes, by cloud_point() and cloud_store() -- where the slot
// lies within the capacity.  (xs, ys) lies inside the grid.
__host__ __device__ __forceinline__ void mesh_store_vertex(const MeshArgs& a, const CloudStreams& s, int32_t* slot_map, int xs,
                                                           int ys, bool is_vertex, int slot) {
  if (slot_map) slot_map[(size_t)ys * a.c.sub_cols + xs] = is_vertex ? slot : -1;
  if (!is_vertex || slot >= s.capacity) return;
  const int x = xs * a.c.filter.stride, y = ys * a.c.filter.stride;
  float p[3];
  cloud_point(a.c.cam, a.c.disp[(size_t)y * a.c.cols + x], x, y, p);
  cloud_store(a.c, s, slot, x, y, p);
}

// The emitted triangles of cell (xs, ys), `cell` being mesh_cell()'s value for it (not 0), into slots `slot` (T0, or T1
// where there is no T0) and slot + 1 (T1 behind a T0), each where it lies within the capacity.
__host__ __device__ __forceinline__ void mesh_store_triangles(const MeshArgs& a, const int32_t* slot_map, int32_t* tri_out,
                                                              int tri_capacity, int xs, int ys, unsigned cell, int slot) {
  const int32_t* m = slot_map + (size_t)ys * a.c.sub_cols + xs;
  const int32_t s00 = m[0], s10 = m[1], s01 = m[a.c.sub_cols], s11 = m[a.c.sub_cols + 1];
  const bool diag1 = (cell & kMeshDiag1) != 0;
  if ((cell & kMeshT0) && slot < tri_capacity) {
    int32_t* o = tri_out + (size_t)slot * 3;
    o[0] = s00, o[1] = s01, o[2] = diag1 ? s10 : s11;
  }
  slot += (int)(cell & kMeshT0);
  if ((cell & kMeshT1) && slot < tri_capacity) {
    int32_t* o = tri_out + (size_t)slot * 3;
    o[0] = diag1 ? s10 : s00, o[1] = diag1 ? s01 : s11, o[2] = diag1 ? s11 : s10;
  }
}

}  // namespace pm
