// pm_tsdf_mesh.hpp -- the kernels of pm_tsdf_mesh (include/pm/imaging.h); included by pm_stages.hip alone.  The case table, the
// arithmetic and the per-thread bodies are pm_tsdf_mesh_body.hpp's, the definition is tests/tsdf_mesh_ref.py (DESIGN.md section
// 8c-11).
//
// A wavefront owns a SPAN, as in k_tsdf_integrate: 64 consecutive nodes along x of one (j, k) row, lane l node l.  The spans are
// numbered x fastest, so span order is the node order and the cell order of the definition, and a block's four wavefronts take
// four consecutive spans.  Seven launches, none of which waits for another workgroup; the span kernels have no barrier, so a
// wavefront behind the last span simply leaves, and inside a wavefront every lane reaches every ballot:
//   k_tsdf_mesh_flags      per node one byte: which of its seven owned edges cross, and whether its cell is live;
//   k_tsdf_mesh_count      per node which crossing edges are vertices (the live bits of the up to eight cells around an edge are
//                          the bytes of the nodes at negative offsets) and how many triangles its cell emits (from the byte
//                          alone: the count of a sign pattern is that of its complement); a lane's vertices are at most 7 and
//                          its triangles at most 12, so its rank in the wavefront is a sum over 3 / 4 bit planes of
//                          mbcnt(ballot(bit)); per node the vertex mask and the rank, per span the two sums;
//   k_tsdf_mesh_span_offsets  a block per GROUP of 1024 consecutive spans: both counts of a span become its exclusive offsets
//                          inside the group (k_cloud_offsets' scan of one pass: wave shuffles, then the wave sums through LDS;
//                          every thread reaches both barriers), and the group's two sums are written;
//   k_cloud_offsets        twice (pm_cloud.hpp, as it stands) over the GROUP sums: exclusive group offsets and the totals.  A
//                          256^3 volume has 262144 spans and 256 groups: one pass of that single-block kernel, not 256;
//   k_tsdf_mesh_vertices   positions and normals; slot = group offset + span offset + rank + set bits of the mask below the edge;
//   k_tsdf_mesh_triangles  the rank of the cell's triangles again; a vertex's slot from its owner's offsets, rank and mask.
// The order is this arithmetic, never an atomic.  Nothing is read outside the volume, nothing written behind a capacity.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_mesh.hpp"
#include "pm_tsdf_mesh_body.hpp"

namespace pm {

// The wavefront's span and the lane's node.  false: the wavefront lies behind the last span (wave-uniform).
__device__ __forceinline__ bool tsdf_mesh_lane(const TsdfMeshArgs& a, unsigned spans, unsigned* span, int* i, int* j, int* k) {
  *span = blockIdx.x * kTsdfBlockY + (unsigned)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
  if (*span >= spans) return false;
  const unsigned row = *span / (unsigned)a.x_spans;
  *i = (int)((*span - row * (unsigned)a.x_spans) * kTsdfLanes + threadIdx.x);
  *k = (int)(row / (unsigned)a.grid.ny);
  *j = (int)(row - (unsigned)*k * (unsigned)a.grid.ny);
  return true;
}

// n < 2^BITS per lane: the sum over the lanes below this one, and over the wavefront.  Every lane of the wavefront gets here.
template <int BITS>
__device__ __forceinline__ void tsdf_mesh_wave_rank(int n, int* rank, int* total) {
  int r = 0, t = 0;
#pragma unroll
  for (int b = 0; b < BITS; ++b) {
    const unsigned long long m = __ballot((n >> b) & 1);
    r += mesh_rank(m) << b;
    t += __popcll(m) << b;
  }
  *rank = r, *total = t;
}

// the span kernels: grid = ceil(spans / 4), block = (64, 4); spans = x_spans * ny * nz
__global__ void __launch_bounds__(kTsdfBlockX * kTsdfBlockY) k_tsdf_mesh_flags(TsdfMeshArgs a, unsigned spans) {
  unsigned span;
  int i, j, k;
  if (!tsdf_mesh_lane(a, spans, &span, &i, &j, &k) || i >= a.grid.nx) return;
  a.flags[tsdf_mesh_node(a.grid, i, j, k)] = (uint8_t)tsdf_mesh_flags_lane(a, i, j, k);
}

__global__ void __launch_bounds__(kTsdfBlockX * kTsdfBlockY) k_tsdf_mesh_count(TsdfMeshArgs a, unsigned spans) {
  unsigned span;
  int i, j, k;
  if (!tsdf_mesh_lane(a, spans, &span, &i, &j, &k)) return;
  const bool in_grid = i < a.grid.nx;
  const size_t node = in_grid ? tsdf_mesh_node(a.grid, i, j, k) : 0;
  const unsigned flags = in_grid ? a.flags[node] : 0u;
  const unsigned mask = in_grid ? tsdf_mesh_vertex_mask(a, i, j, k, flags) : 0u;
  int v_rank, v_total, t_rank, t_total;
  tsdf_mesh_wave_rank<3>(__builtin_popcount(mask), &v_rank, &v_total);
  tsdf_mesh_wave_rank<4>(tsdf_mesh_triangles_of(flags), &t_rank, &t_total);
  if (in_grid) a.info[node] = mask | ((uint32_t)v_rank << 8);
  if (threadIdx.x == 0) a.vertex_spans[span] = v_total, a.tri_spans[span] = t_total;
}

// grid = ceil(spans / kTsdfMeshGroup), block = kTsdfMeshGroup.  vertex_spans and tri_spans of the block's group -> exclusive offsets
// inside the group, in place; vertex_groups[blockIdx.x], tri_groups[blockIdx.x] = the group's sums.
__global__ void __launch_bounds__(kTsdfMeshGroup) k_tsdf_mesh_span_offsets(TsdfMeshArgs a, unsigned spans) {
  constexpr int kWaves = kTsdfMeshGroup / 64;
  __shared__ int wave_sum[2][kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned span = blockIdx.x * kTsdfMeshGroup + threadIdx.x;
  const int v = span < spans ? a.vertex_spans[span] : 0, t = span < spans ? a.tri_spans[span] : 0;
  int v_incl = v, t_incl = t;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {  // every thread of the block: no early exit in front of a shuffle or the barrier
    const int pv = __shfl_up(v_incl, o), pt = __shfl_up(t_incl, o);
    if (lane >= o) v_incl += pv, t_incl += pt;
  }
  if (lane == 63) wave_sum[0][wave] = v_incl, wave_sum[1][wave] = t_incl;
  __syncthreads();
  int v_before = 0, v_all = 0, t_before = 0, t_all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int sv = wave_sum[0][w], st = wave_sum[1][w];
    v_before += w < wave ? sv : 0, t_before += w < wave ? st : 0;
    v_all += sv, t_all += st;
  }
  if (span < spans) a.vertex_spans[span] = v_before + (v_incl - v), a.tri_spans[span] = t_before + (t_incl - t);
  if (threadIdx.x == 0) a.vertex_groups[blockIdx.x] = v_all, a.tri_groups[blockIdx.x] = t_all;
}

// behind the scans
__global__ void __launch_bounds__(kTsdfBlockX * kTsdfBlockY) k_tsdf_mesh_vertices(TsdfMeshArgs a, unsigned spans) {
  unsigned span;
  int i, j, k;
  if (!tsdf_mesh_lane(a, spans, &span, &i, &j, &k) || i >= a.grid.nx) return;
  tsdf_mesh_vertices_lane(a, i, j, k);
}

// behind the scans
__global__ void __launch_bounds__(kTsdfBlockX * kTsdfBlockY) k_tsdf_mesh_triangles(TsdfMeshArgs a, unsigned spans) {
  unsigned span;
  int i, j, k;
  if (!tsdf_mesh_lane(a, spans, &span, &i, &j, &k)) return;
  const int n = i < a.grid.nx ? tsdf_mesh_triangles_of(a.flags[tsdf_mesh_node(a.grid, i, j, k)]) : 0;
  int rank, total;
  tsdf_mesh_wave_rank<4>(n, &rank, &total);
  if (n) tsdf_mesh_triangles_lane(a, i, j, k, tsdf_mesh_tri_offset(a, span) + rank);  // a cell with a triangle is live: inside the grid
}

}  // namespace pm
