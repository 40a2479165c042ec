// pm_mesh.hpp -- the kernels of pm_grid_mesh (include/pm/imaging.h); included by pm_stages.hip alone.  The arithmetic
// and the per-thread bodies (mesh_value, mesh_cell, mesh_referenced, mesh_store_vertex, mesh_store_triangles) are
// pm_mesh_body.hpp's, the definition is tests/mesh_ref.py.
//
// A block of kMeshBlock threads owns kMeshBlock consecutive items of ONE row of the stride grid, so blocks in
// (row, segment) order are the row-major order of the items and of the cells.  It stages the VALUES (mesh_value: the
// disparity where the item counts, 0 elsewhere and outside the grid) of the rows it needs, with one item either side, in
// LDS; the 2x2 cells then read LDS, and the 3x3 test of the REFERENCED vertices reads the four cells around its item,
// which the block evaluates once each and shares through LDS.  Five launches, none of which waits for another workgroup:
//   k_mesh_count      per block: its vertices (one ballot) and its triangles (two ballots: T0 and T1 of the lanes' cells);
//   k_cloud_offsets   twice (pm_cloud.hpp, as it stands): exclusive block offsets and the total, for each of the two;
//   k_mesh_vertices   the vertex predicate again; slot = block offset + wavefronts in front + rank under the ballot mask;
//                     writes the organised slot map for every item and the vertex streams within the capacity;
//   k_mesh_triangles  the cell predicate again; a lane's rank is the set bits of BOTH masks below it, its T1 goes behind
//                     its own T0; the three vertex slots of a triangle are read from the slot map.
// The order is this arithmetic, never an atomic.  Every thread of a block reaches every barrier and ballot.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_cloud.hpp"
#include "pm_mesh_body.hpp"

namespace pm {

constexpr int kMeshBlock = 256;  // items of a grid row per block: four wavefronts

// blocks per grid row
inline int mesh_segments(int sub_cols) { return (sub_cols + kMeshBlock - 1) / kMeshBlock; }

// The staged values of a block: row dy + 1 holds grid row ys + dy, column k + 1 holds item xs0 + k, k = -1 .. kMeshBlock.
// cell[r][k]: mesh_cell() of the cell whose corner 00 is item xs0 + k - 1 of grid row ys + r - 1 (REFERENCED vertices only).
struct MeshTile {
  float v[3][kMeshBlock + 2];
  uint8_t cell[2][kMeshBlock + 1];
};

// The block's position: its grid row and the first item of its segment.
__device__ __forceinline__ void mesh_block(const MeshArgs& a, int* ys, int* xs0) {
  const int segments = (a.c.sub_cols + kMeshBlock - 1) / kMeshBlock;
  *ys = (int)(blockIdx.x / (unsigned)segments);
  *xs0 = (int)(blockIdx.x % (unsigned)segments) * kMeshBlock;
}

// Rows ys + dy_lo .. ys + dy_hi of the block's segment into the tile, then the barrier.  Rows that are not asked for stay
// unwritten and are not read.
__device__ __forceinline__ void mesh_stage(const MeshArgs& a, MeshTile& t, int ys, int xs0, int dy_lo, int dy_hi) {
  for (int dy = dy_lo; dy <= dy_hi; ++dy) {  // uniform bounds
    t.v[dy + 1][threadIdx.x + 1] = mesh_value(a, xs0 + (int)threadIdx.x, ys + dy);
    if (threadIdx.x < 2) {
      const int k = threadIdx.x ? kMeshBlock : -1;
      t.v[dy + 1][k + 1] = mesh_value(a, xs0 + k, ys + dy);
    }
  }
  __syncthreads();
}

// mesh_cell() of the cell whose corner 00 is item xs0 + k - 1 of grid row ys + r - 1; rows r and r + 1 of the tile are staged.
__device__ __forceinline__ unsigned mesh_tile_cell(const MeshArgs& a, const MeshTile& t, int r, int k) {
  return mesh_cell(t.v[r][k], t.v[r][k + 1], t.v[r + 1][k], t.v[r + 1][k + 1], a.max_diff);
}

// mesh_cell() of the cell whose corner 00 is the thread's item.  Rows ys and ys + 1 are staged.
__device__ __forceinline__ unsigned mesh_thread_cell(const MeshArgs& a, const MeshTile& t) {
  return mesh_tile_cell(a, t, 1, (int)threadIdx.x + 1);
}

// Whether the thread's item is a vertex.  REFERENCED: rows ys - 1 .. ys + 1 are staged and `own` is mesh_thread_cell();
// every thread evaluates its own cell and the one above once, two threads the pair left of the segment, and the four cells
// around an item meet in LDS behind a barrier every thread of the block reaches (a.referenced is the launch's).
__device__ __forceinline__ bool mesh_thread_vertex(const MeshArgs& a, MeshTile& t, unsigned own) {
  const int k = (int)threadIdx.x + 1;
  if (!a.referenced) return t.v[1][k] > 0.f;
  t.cell[0][k] = (uint8_t)mesh_tile_cell(a, t, 0, k);
  t.cell[1][k] = (uint8_t)own;
  if (threadIdx.x < 2) t.cell[threadIdx.x][0] = (uint8_t)mesh_tile_cell(a, t, (int)threadIdx.x, 0);
  __syncthreads();
  return t.v[1][k] > 0.f && mesh_referenced_cells(t.cell[0][k - 1], t.cell[0][k], t.cell[1][k - 1], t.cell[1][k]);
}

__device__ __forceinline__ int mesh_rank(unsigned long long mask) {  // the set bits of the mask below the lane
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// grid = sub_rows * mesh_segments(sub_cols), block = kMeshBlock.  vertex_counts[b], tri_counts[b]: those of block b.
__global__ void __launch_bounds__(kMeshBlock) k_mesh_count(MeshArgs a, int* __restrict__ vertex_counts,
                                                           int* __restrict__ tri_counts) {
  __shared__ MeshTile tile;
  __shared__ int wave_count[2][kMeshBlock / 64];
  int ys, xs0;
  mesh_block(a, &ys, &xs0);
  mesh_stage(a, tile, ys, xs0, a.referenced ? -1 : 0, 1);
  const unsigned cell = mesh_thread_cell(a, tile);
  const unsigned long long vm = __ballot(mesh_thread_vertex(a, tile, cell));
  const unsigned long long m0 = __ballot((cell & kMeshT0) != 0), m1 = __ballot((cell & kMeshT1) != 0);
  if ((threadIdx.x & 63) == 0) {
    wave_count[0][threadIdx.x >> 6] = __popcll(vm);
    wave_count[1][threadIdx.x >> 6] = __popcll(m0) + __popcll(m1);
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kMeshBlock / 64; ++w) sum += wave_count[threadIdx.x][w];
    (threadIdx.x ? tri_counts : vertex_counts)[blockIdx.x] = sum;
  }
}

// grid and block as k_mesh_count; offsets: what k_cloud_offsets left of vertex_counts.  slot_map: [sub_rows][sub_cols].
__global__ void __launch_bounds__(kMeshBlock) k_mesh_vertices(MeshArgs a, const int* __restrict__ offsets, CloudStreams s,
                                                              int32_t* __restrict__ slot_map) {
  __shared__ MeshTile tile;
  __shared__ int wave_count[kMeshBlock / 64];
  int ys, xs0;
  mesh_block(a, &ys, &xs0);
  mesh_stage(a, tile, ys, xs0, a.referenced ? -1 : 0, a.referenced ? 1 : 0);
  const bool is_vertex = mesh_thread_vertex(a, tile, a.referenced ? mesh_thread_cell(a, tile) : 0u);
  const unsigned long long mask = __ballot(is_vertex);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wave_count[wave] = __popcll(mask);
  __syncthreads();
  int slot = offsets[blockIdx.x] + mesh_rank(mask);
#pragma unroll
  for (int w = 0; w < kMeshBlock / 64; ++w) slot += w < wave ? wave_count[w] : 0;
  const int xs = xs0 + (int)threadIdx.x;
  if (xs < a.c.sub_cols) mesh_store_vertex(a, s, slot_map, xs, ys, is_vertex, slot);
}

// grid and block as k_mesh_count; offsets: what k_cloud_offsets left of tri_counts; slot_map: what k_mesh_vertices wrote.
__global__ void __launch_bounds__(kMeshBlock) k_mesh_triangles(MeshArgs a, const int* __restrict__ offsets,
                                                               const int32_t* __restrict__ slot_map, int32_t* __restrict__ tri_out,
                                                               int tri_capacity) {
  __shared__ MeshTile tile;
  __shared__ int wave_count[kMeshBlock / 64];
  int ys, xs0;
  mesh_block(a, &ys, &xs0);
  mesh_stage(a, tile, ys, xs0, 0, 1);
  const unsigned cell = mesh_thread_cell(a, tile);
  const unsigned long long m0 = __ballot((cell & kMeshT0) != 0), m1 = __ballot((cell & kMeshT1) != 0);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wave_count[wave] = __popcll(m0) + __popcll(m1);
  __syncthreads();
  int slot = offsets[blockIdx.x] + mesh_rank(m0) + mesh_rank(m1);
#pragma unroll
  for (int w = 0; w < kMeshBlock / 64; ++w) slot += w < wave ? wave_count[w] : 0;
  // a cell with a triangle lies inside the grid: the values outside it are 0
  if (cell & (kMeshT0 | kMeshT1)) mesh_store_triangles(a, slot_map, tri_out, tri_capacity, xs0 + (int)threadIdx.x, ys, cell, slot);
}

}  // namespace pm
