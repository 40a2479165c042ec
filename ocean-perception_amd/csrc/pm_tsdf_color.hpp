// pm_tsdf_color.hpp -- the kernels of pm_tsdf_integrate_color, pm_tsdf_color_map and pm_tsdf_color_points
// (include/pm/imaging.h; pm_tsdf_color_clear is a memset); included by pm_stages.hip alone.  The arithmetic and the per-thread
// bodies are pm_tsdf_color_body.hpp's, the definition is tests/tsdf_color_ref.py.
//
//   k_tsdf_integrate_color  k_tsdf_integrate's walk (pm_tsdf.hpp: a wavefront per 64 voxels along x, the stride loop with a
//                           wave-uniform trip count, the arguments by value in scalar registers, the counts by ballot, one
//                           integer add per block and counter) with a third counter.  The distance arithmetic is
//                           tsdf_integrate_lane's one statement; a voxel that survived every test and lies in the band loads
//                           its pixel's three bytes or floats and its 16-byte colour record, and stores the record.  No voxel
//                           is touched by two threads: no atomics on either volume.
//   k_tsdf_color_map        one pixel per lane, 64 consecutive pixels of a row per wavefront, four rows per block.
//   k_tsdf_color_points     one point per lane, 256 consecutive points per block; *d_n is read through a wave-uniform address.
//                           Both gathers: eight 16-byte corner loads, each behind the test that the corner lies in the grid;
//                           the count is k_tsdf_raycast's tail (tsdf_block_count).
// Every thread of a block reaches every ballot and the barrier.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_tsdf.hpp"
#include "pm_tsdf_color_body.hpp"

namespace pm {

static_assert(sizeof(TsdfColor) == 16 && alignof(TsdfColor) == 16, "a colour record is one 16-byte access");
static_assert(sizeof(TsdfIntegrateColorArgs) <= 320 && sizeof(TsdfColorMapArgs) <= 320 && sizeof(TsdfColorPointsArgs) <= 160,
              "the by-value arguments stay small");

// grid = (min(ceil(spans / 4), kTsdfMaxBlocks)), block = (64, 4); spans = ceil(nx / 64) * ny * nz
// (k_tsdf_integrate's walk with a third counter: the two change together.)
__global__ void __launch_bounds__(kTsdfBlockX * kTsdfBlockY) k_tsdf_integrate_color(TsdfIntegrateColorArgs a) {
  __shared__ int wave_counts[kTsdfBlockY][3];
  const TsdfGrid& g = a.base.grid;
  const unsigned x_spans = ((unsigned)g.nx + kTsdfLanes - 1) / kTsdfLanes;
  const unsigned long long spans = (unsigned long long)x_spans * (unsigned)g.ny * (unsigned)g.nz;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
  int in_view = 0, updated = 0, colored = 0;
  for (unsigned long long s = (unsigned long long)blockIdx.x * kTsdfBlockY + wave; s < spans;
       s += (unsigned long long)gridDim.x * kTsdfBlockY) {  // wave-uniform: nobody leaves in front of a ballot
    const unsigned long long row = s / x_spans;
    const int i = (int)((unsigned)(s - row * x_spans) * kTsdfLanes + threadIdx.x);
    const int k = (int)(row / (unsigned)g.ny);
    const int j = (int)(row - (unsigned long long)k * (unsigned)g.ny);
    const unsigned flags = i < g.nx ? tsdf_integrate_color_lane(a, i, j, k) : 0u;
    in_view += __popcll(__ballot(flags & 1u));
    updated += __popcll(__ballot((flags >> 1) & 1u));
    colored += __popcll(__ballot((flags >> 2) & 1u));
  }
  if (threadIdx.x == 0) wave_counts[threadIdx.y][0] = in_view, wave_counts[threadIdx.y][1] = updated, wave_counts[threadIdx.y][2] = colored;
  __syncthreads();
  if (threadIdx.x < 3 && threadIdx.y == 0) {  // lane c: counter c
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kTsdfBlockY; ++w) sum += wave_counts[w][threadIdx.x];
    if (sum) reproject_add(a.base.counts + threadIdx.x, sum);
  }
}

// grid = (ceil(cols / 64), ceil(rows / 4)), block = (64, 4)
__global__ void __launch_bounds__(kTsdfBlockX * kTsdfBlockY) k_tsdf_color_map(TsdfColorMapArgs a) {
  const int x = (int)(blockIdx.x * kTsdfLanes + threadIdx.x);
  const int y = (int)(blockIdx.y * kTsdfBlockY + threadIdx.y);
  const bool colored = x < a.cols && y < a.rows ? tsdf_color_map_lane(a, x, y) : false;  // nobody leaves in front of the ballot
  tsdf_block_count(colored, a.s.counts);
}

// grid = (ceil(n / 256)), block = (64, 4)
__global__ void __launch_bounds__(kTsdfBlockX * kTsdfBlockY) k_tsdf_color_points(TsdfColorPointsArgs a) {
  const int limit = __builtin_amdgcn_readfirstlane(tsdf_color_points_limit(a));  // once per wavefront
  const long long at = ((long long)blockIdx.x * kTsdfBlockY + threadIdx.y) * kTsdfLanes + threadIdx.x;
  const bool colored = at < (long long)limit ? tsdf_color_point_lane(a, (int)at) : false;
  tsdf_block_count(colored, a.s.counts);
}

}  // namespace pm
