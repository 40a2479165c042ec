// pm_tsdf_mesh_body.hpp -- the case table, the arithmetic and the per-thread bodies of pm_tsdf_mesh (include/pm/imaging.h),
// host-callable and free of kernels, so that the kernels (pm_tsdf_mesh.hpp) and a CPU build (tests/cpp/tsdf_mesh_host_main.cpp,
// under the sanitizers) share ONE statement of it.  The definition it is held to BIT FOR BIT is tests/tsdf_mesh_ref.py (DESIGN.md
// section 8c-11): marching tetrahedra over the Kuhn split of every cell into six tetrahedra around the diagonal 000-111, one
// vertex per crossed grid edge.  Every operation is one rounding in the format written, parentheses as written.
//
// Numbers used throughout: a CORNER of a cell is 0..7, bit 0 x, bit 1 y, bit 2 z.  Node a owns the seven EDGES a -> a + d; edge
// e = 0..6 has the direction corner tsdf_mesh_edge_dir(e) = 1, 2, 4, 3, 6, 5, 7 (the cube edges along x, y, z, the face diagonals
// xy, yz, xz, the main diagonal).  A vertex CODE is (corner of the owning node inside the cell) | (edge number << 3).
// A SPAN is 64 consecutive nodes along x of one (j, k) row; the spans are numbered x fastest, so span order is node order.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_tsdf_body.hpp"

namespace pm {

constexpr int kTsdfMeshMaxCellTriangles = 12;  // two per tetrahedron
constexpr unsigned kTsdfMeshLive = 0x80u;      // bit 7 of a node's flag byte: the cell whose corner 0 the node is, is live
constexpr int kTsdfMeshGroup = 1024;           // spans whose counts one block of k_tsdf_mesh_span_offsets scans

__host__ __device__ constexpr unsigned tsdf_mesh_edge_dir(int e) { return (0x7563421u >> (4 * e)) & 7u; }
// the edge number of the direction corner d = 1..7
__host__ __device__ constexpr unsigned tsdf_mesh_dir_edge(unsigned d) { return (0x64523100u >> (4 * d)) & 7u; }
// corners 1 and 2 of tetrahedron t = 0..5 (the axis orders xyz, xzy, yxz, yzx, zxy, zyx); corner 0 is 0 and corner 3 is 7
__host__ __device__ constexpr unsigned tsdf_mesh_tet_corner(int t, int n) {
  return n == 0 ? 0u : n == 3 ? 7u : ((n == 1 ? 0x442211u : 0x656353u) >> (4 * t)) & 7u;
}

// One tetrahedron under one pattern of its four corners (bit n: corner n inside): n triangles of three vertex codes.
struct TsdfMeshTetCase {
  uint8_t n;
  uint8_t v[6];
};
struct TsdfMeshTable {
  TsdfMeshTetCase tet[6][16];
};

// The table, DERIVED from the definition's integer rule (nothing of it is typed in).  I: the inside corners, O: the outside ones.
// |I| = 1, I = {a}: the polygon is the edges (a, o), o ascending; |I| = 3, O = {a}: (i, a), i ascending; |I| = 2, I = {a < b},
// O = {c < d}: (a, c), (a, d), (b, d), (b, c).  With the polygon's vertices at their edges' midpoints in doubled corner
// coordinates, it is read back to front iff ((Q1 - Q0) x (Q2 - Q0)) . (|I| sum(O) - |O| sum(I)) < 0.  Triangles (q0, q1, q2) and
// (q0, q2, q3).
constexpr TsdfMeshTable tsdf_mesh_make_table() {
  TsdfMeshTable table = {};
  for (int t = 0; t < 6; ++t)
    for (int pattern = 1; pattern < 15; ++pattern) {
      int in[4] = {}, out[4] = {}, n_in = 0, n_out = 0;
      for (int c = 0; c < 4; ++c) {
        if ((pattern >> c) & 1) in[n_in++] = c;
        else out[n_out++] = c;
      }
      int pu[4] = {}, pv[4] = {}, n = 0;  // the polygon's edges between corners pu and pv of the tetrahedron
      if (n_in == 1) {
        for (int o = 0; o < 3; ++o) pu[n] = in[0], pv[n] = out[o], ++n;
      } else if (n_in == 3) {
        for (int i = 0; i < 3; ++i) pu[n] = in[i], pv[n] = out[0], ++n;
      } else {
        pu[0] = in[0], pv[0] = out[0], pu[1] = in[0], pv[1] = out[1], pu[2] = in[1], pv[2] = out[1], pu[3] = in[1], pv[3] = out[0];
        n = 4;
      }
      int P[4][3] = {};
      for (int c = 0; c < 4; ++c)
        for (int x = 0; x < 3; ++x) P[c][x] = (int)((tsdf_mesh_tet_corner(t, c) >> x) & 1u);
      int Q[3][3] = {}, side[3] = {};
      for (int q = 0; q < 3; ++q)
        for (int x = 0; x < 3; ++x) Q[q][x] = P[pu[q]][x] + P[pv[q]][x];
      for (int x = 0; x < 3; ++x) {
        for (int o = 0; o < n_out; ++o) side[x] += n_in * P[out[o]][x];
        for (int i = 0; i < n_in; ++i) side[x] -= n_out * P[in[i]][x];
      }
      const int a[3] = {Q[1][0] - Q[0][0], Q[1][1] - Q[0][1], Q[1][2] - Q[0][2]};
      const int b[3] = {Q[2][0] - Q[0][0], Q[2][1] - Q[0][1], Q[2][2] - Q[0][2]};
      const int value = (a[1] * b[2] - a[2] * b[1]) * side[0] + (a[2] * b[0] - a[0] * b[2]) * side[1] + (a[0] * b[1] - a[1] * b[0]) * side[2];
      uint8_t code[4] = {};
      for (int q = 0; q < n; ++q) {
        const int at = value < 0 ? n - 1 - q : q;
        const unsigned lo = tsdf_mesh_tet_corner(t, pu[at] < pv[at] ? pu[at] : pv[at]);
        const unsigned hi = tsdf_mesh_tet_corner(t, pu[at] < pv[at] ? pv[at] : pu[at]);
        code[q] = (uint8_t)(lo | (tsdf_mesh_dir_edge(hi ^ lo) << 3));  // the corners of a tetrahedron ascend: hi - lo = hi ^ lo
      }
      TsdfMeshTetCase& o = table.tet[t][pattern];
      o.n = (uint8_t)(n - 2);
      o.v[0] = code[0], o.v[1] = code[1], o.v[2] = code[2];
      if (n == 4) o.v[3] = code[0], o.v[4] = code[2], o.v[5] = code[3];
    }
  return table;
}
constexpr TsdfMeshTable kTsdfMeshTable = tsdf_mesh_make_table();

// The pattern of tetrahedron t's four corners out of the cell's eight inside bits.
__host__ __device__ __forceinline__ unsigned tsdf_mesh_tet_pattern(unsigned pattern8, int t) {
  return (pattern8 & 1u) | (((pattern8 >> tsdf_mesh_tet_corner(t, 1)) & 1u) << 1) | (((pattern8 >> tsdf_mesh_tet_corner(t, 2)) & 1u) << 2) |
         (((pattern8 >> 7) & 1u) << 3);
}

// The triangles of a cell with the inside bits pattern8, in the definition's order: emit(code0, code1, code2) for each.
template <typename Emit>
__host__ __device__ __forceinline__ void tsdf_mesh_cell_triangles(unsigned pattern8, Emit emit) {
#pragma unroll 1
  for (int t = 0; t < 6; ++t) {
    const TsdfMeshTetCase& c = kTsdfMeshTable.tet[t][tsdf_mesh_tet_pattern(pattern8, t)];
    if (c.n >= 1) emit(c.v[0], c.v[1], c.v[2]);
    if (c.n >= 2) emit(c.v[3], c.v[4], c.v[5]);
  }
}

// How many that is.  The count does not change when every bit of the pattern is inverted.
__host__ __device__ __forceinline__ int tsdf_mesh_cell_triangle_count(unsigned pattern8) {
  int n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const int inside = __builtin_popcount(tsdf_mesh_tet_pattern(pattern8, t));
    n += inside == 2 ? 2 : (inside == 1 || inside == 3) ? 1 : 0;
  }
  return n;
}

// ---- what the launches share ---------------------------------------------------------------------------------------------------
// The scratch: flags, one byte per node (bits 0-6: the node's owned edges cross, bit 7: its cell is live); info, one word per node
// (bits 0-6: which owned edges are vertices, bits 8..: the vertices of the node's span in front of the node); one word per span
// for the vertices and one for the triangles (its count, then its offset inside its GROUP of kTsdfMeshGroup consecutive spans); one
// word per group for each of the two (its count, then its offset).
struct TsdfMeshArgs {
  TsdfGrid grid;
  float min_weight;
  int x_spans;  // ceil(nx / 64)
  const TsdfVoxel* voxels;
  uint8_t* flags;
  uint32_t* info;
  int* vertex_spans;
  int* tri_spans;
  int* vertex_groups;  // one word per kTsdfMeshGroup spans for the vertices and one for the triangles (its count, then its offset)
  int* tri_groups;
  float* xyz_out;      // [vertex_capacity][3]; may be null
  float* normals_out;  // [vertex_capacity][3]; may be null
  int32_t* tri_out;    // [tri_capacity][3]; may be null
  int vertex_capacity, tri_capacity;
};

__host__ __device__ __forceinline__ size_t tsdf_mesh_node(const TsdfGrid& g, int i, int j, int k) {
  return ((size_t)k * g.ny + j) * g.nx + i;
}
__host__ __device__ __forceinline__ size_t tsdf_mesh_span(const TsdfMeshArgs& a, int i, int j, int k) {
  return ((size_t)k * a.grid.ny + j) * a.x_spans + (size_t)(i / kTsdfLanes);
}

// Node (i, j, k), anywhere: 0 outside the grid or not OBSERVED (weight > 0, weight >= min_weight, tsdf finite), 1 observed and
// outside the surface (tsdf > 0), 3 observed and INSIDE.  *tsdf: its value, 0 outside the grid.  Nothing outside the volume is read.
__host__ __device__ __forceinline__ unsigned tsdf_mesh_state(const TsdfMeshArgs& a, int i, int j, int k, float* tsdf) {
  *tsdf = 0.f;
  if (i < 0 || j < 0 || k < 0 || i >= a.grid.nx || j >= a.grid.ny || k >= a.grid.nz) return 0u;
  const TsdfVoxel v = a.voxels[tsdf_mesh_node(a.grid, i, j, k)];
  *tsdf = v.tsdf;
  const bool observed = v.weight > 0.f && v.weight >= a.min_weight && __builtin_fabsf(v.tsdf) < __builtin_inff();
  return !observed ? 0u : v.tsdf > 0.f ? 1u : 3u;
}

// k_tsdf_mesh_flags, node (i, j, k) inside the grid: its flag byte, from the states of the eight corners of its cell.
__host__ __device__ __forceinline__ unsigned tsdf_mesh_flags_lane(const TsdfMeshArgs& a, int i, int j, int k) {
  float unused;
  const unsigned s0 = tsdf_mesh_state(a, i, j, k, &unused);
  unsigned flags = 0u, all = s0 & 1u;
#pragma unroll
  for (int e = 0; e < 7; ++e) {
    const unsigned d = tsdf_mesh_edge_dir(e);
    const unsigned s = tsdf_mesh_state(a, i + (int)(d & 1u), j + (int)((d >> 1) & 1u), k + (int)(d >> 2), &unused);
    all &= s;
    if ((s0 & s & 1u) && ((s0 ^ s) & 2u)) flags |= 1u << e;  // both observed, exactly one inside
  }
  return flags | (all ? kTsdfMeshLive : 0u);
}

// The inside bits of a live cell's corners 1..7 relative to corner 0 (bit 0 is 0): what the flag byte knows of them.
__host__ __device__ __forceinline__ unsigned tsdf_mesh_relative_pattern(unsigned flags) {
  unsigned p = 0u;
#pragma unroll
  for (unsigned c = 1; c < 8; ++c) p |= ((flags >> tsdf_mesh_dir_edge(c)) & 1u) << c;
  return p;
}

// The triangles of the cell whose flag byte is `flags`.
__host__ __device__ __forceinline__ int tsdf_mesh_triangles_of(unsigned flags) {
  return (flags & kTsdfMeshLive) ? tsdf_mesh_cell_triangle_count(tsdf_mesh_relative_pattern(flags)) : 0;
}

// k_tsdf_mesh_count, node (i, j, k) inside the grid: which of its crossing edges lie in a live cell.  Edge e lies in the cells
// whose corner 0 is the node minus s, s over the subsets of the axes on which the edge's direction is 0.
__host__ __device__ __forceinline__ unsigned tsdf_mesh_vertex_mask(const TsdfMeshArgs& a, int i, int j, int k, unsigned flags) {
  if (!(flags & 0x7fu)) return 0u;
  unsigned live = 0u;  // bit s: the cell at the node minus s is live
#pragma unroll
  for (unsigned s = 0; s < 8; ++s) {
    const int ci = i - (int)(s & 1u), cj = j - (int)((s >> 1) & 1u), ck = k - (int)(s >> 2);
    if (ci >= 0 && cj >= 0 && ck >= 0 && (a.flags[tsdf_mesh_node(a.grid, ci, cj, ck)] & kTsdfMeshLive)) live |= 1u << s;
  }
  unsigned mask = 0u;
#pragma unroll
  for (int e = 0; e < 7; ++e) {
    const unsigned free_axes = ~tsdf_mesh_edge_dir(e) & 7u;
    bool in_live = false;
#pragma unroll
    for (unsigned s = 0; s < 8; ++s) in_live = in_live || ((s & ~free_axes) == 0u && ((live >> s) & 1u));
    if (((flags >> e) & 1u) && in_live) mask |= 1u << e;
  }
  return mask;
}

// The vertices in front of a span and the triangles in front of it, behind the scans: its group's offset and its own inside it.
__host__ __device__ __forceinline__ int tsdf_mesh_vertex_offset(const TsdfMeshArgs& a, size_t span) {
  return a.vertex_groups[span / kTsdfMeshGroup] + a.vertex_spans[span];
}
__host__ __device__ __forceinline__ int tsdf_mesh_tri_offset(const TsdfMeshArgs& a, size_t span) {
  return a.tri_groups[span / kTsdfMeshGroup] + a.tri_spans[span];
}

// The slot of the vertex on edge e of node (i, j, k), which is one.
__host__ __device__ __forceinline__ int tsdf_mesh_slot(const TsdfMeshArgs& a, int i, int j, int k, unsigned e) {
  const uint32_t info = a.info[tsdf_mesh_node(a.grid, i, j, k)];
  return tsdf_mesh_vertex_offset(a, tsdf_mesh_span(a, i, j, k)) + (int)(info >> 8) + __builtin_popcount(info & ((1u << e) - 1u));
}

// G_c = T(n + e_c) - T(n - e_c) in binary32; false unless the six neighbours lie inside the grid and are observed.
__host__ __device__ __forceinline__ bool tsdf_mesh_gradient(const TsdfMeshArgs& a, int i, int j, int k, float G[3]) {
  bool valid = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float plus, minus;
    const unsigned sp = tsdf_mesh_state(a, i + (c == 0), j + (c == 1), k + (c == 2), &plus);
    const unsigned sm = tsdf_mesh_state(a, i - (c == 0), j - (c == 1), k - (c == 2), &minus);
    valid = valid && sp && sm;
    G[c] = plus - minus;
  }
  return valid;
}

// k_tsdf_mesh_vertices, node (i, j, k) inside the grid: the positions and the normals of its vertices, each where its slot lies
// within the capacity.
__host__ __device__ __forceinline__ void tsdf_mesh_vertices_lane(const TsdfMeshArgs& a, int i, int j, int k) {
  const size_t node = tsdf_mesh_node(a.grid, i, j, k);
  const uint32_t info = a.info[node];
  const unsigned mask = info & 0x7fu;
  if (!mask) return;
  const int base = tsdf_mesh_vertex_offset(a, tsdf_mesh_span(a, i, j, k)) + (int)(info >> 8);
  if (base >= a.vertex_capacity) return;
  const double fa = (double)a.voxels[node].tsdf;
  const int at[3] = {i, j, k};
  float Ga[3] = {0.f, 0.f, 0.f};
  const bool valid_a = a.normals_out ? tsdf_mesh_gradient(a, i, j, k, Ga) : false;
  int slot = base;
#pragma unroll 1
  for (int e = 0; e < 7; ++e) {
    if (!((mask >> e) & 1u)) continue;
    if (slot >= a.vertex_capacity) return;  // the slots of a node ascend
    const unsigned d = tsdf_mesh_edge_dir(e);
    const int bi = i + (int)(d & 1u), bj = j + (int)((d >> 1) & 1u), bk = k + (int)(d >> 2);
    const double fb = (double)a.voxels[tsdf_mesh_node(a.grid, bi, bj, bk)].tsdf;
    const double t = fa / (fa - fb);
    if (a.xyz_out) {
      float* o = a.xyz_out + (size_t)slot * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (float)(a.grid.origin[c] + (((double)at[c] + (((d >> c) & 1u) ? t : 0.0)) * a.grid.voxel));
    }
    if (a.normals_out) {
      float Gb[3];
      const bool valid_b = tsdf_mesh_gradient(a, bi, bj, bk, Gb);
      float n[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) n[c] = (float)((double)Ga[c] + (t * ((double)Gb[c] - (double)Ga[c])));
      const float l = __builtin_sqrtf(((n[0] * n[0]) + (n[1] * n[1])) + (n[2] * n[2]));
      const bool ok = valid_a && valid_b && l > 0.f && l < __builtin_inff();
      const float q = ok ? l : 1.f;
      float* o = a.normals_out + (size_t)slot * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = ok ? n[c] / q : 0.f;
    }
    ++slot;
  }
}

// k_tsdf_mesh_triangles, the live cell whose corner 0 is node (i, j, k): its triangles into slot `slot` and the following, each
// where it lies within the capacity; a vertex is named by the slot its owner's info gives it.
__host__ __device__ __forceinline__ void tsdf_mesh_triangles_lane(const TsdfMeshArgs& a, int i, int j, int k, int slot) {
  const size_t node = tsdf_mesh_node(a.grid, i, j, k);
  const unsigned relative = tsdf_mesh_relative_pattern(a.flags[node]);
  const unsigned pattern8 = a.voxels[node].tsdf > 0.f ? relative : ~relative & 0xffu;
  tsdf_mesh_cell_triangles(pattern8, [&](unsigned c0, unsigned c1, unsigned c2) {
    if (slot < a.tri_capacity) {
      const unsigned code[3] = {c0, c1, c2};
      int32_t* o = a.tri_out + (size_t)slot * 3;
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const unsigned corner = code[m] & 7u;
        o[m] = tsdf_mesh_slot(a, i + (int)(corner & 1u), j + (int)((corner >> 1) & 1u), k + (int)(corner >> 2), code[m] >> 3);
      }
    }
    ++slot;
  });
}

}  // namespace pm
