// pm_tsdf.hpp -- the kernels of pm_tsdf_integrate and pm_tsdf_raycast (include/pm/imaging.h; pm_tsdf_clear is a memset);
// included by pm_stages.hip alone.  The arithmetic and the per-thread bodies (tsdf_integrate_lane, tsdf_sample, tsdf_ray_lane) are
// pm_tsdf_body.hpp's, the definition is tests/tsdf_ref.py.
//
//   k_tsdf_integrate  a wavefront owns a SPAN: 64 consecutive voxels along x of one (j, k) row of the grid, lane l voxel l, so a
//                     span's records are 512 contiguous bytes read and written with 8-byte accesses.  The spans are numbered
//                     x-fastest and dealt to the wavefronts of the grid in a stride loop whose trip count is wave-uniform.  The
//                     camera, the grid and the pose arrive by value and are wave-uniform: scalar registers.  A voxel loads its
//                     record only after it has survived the projection and the disparity lookup, so a span outside the view or
//                     behind the band touches no volume memory at all.  The two counts go by wavefront ballot into registers,
//                     the four wavefronts meet in LDS behind the loop, and ONE integer add per block and counter reaches memory
//                     (k_fuse's tail).  No voxel is touched by two threads: no atomics on the volume, no cross-workgroup waits.
//   k_tsdf_raycast    one pixel per lane, 64 consecutive pixels of a row per wavefront, four rows per block.  The march is the
//                     plain one: every sample of the definition, in order; a sample outside the grid costs its coordinates
//                     and no load.  The count as above.
// Every thread of a block reaches every ballot and the barrier.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_tsdf_body.hpp"

namespace pm {

// the block (kTsdfBlockX, kTsdfBlockY) is pm_tsdf_body.hpp's, where a CPU build reads it too
constexpr unsigned kTsdfMaxBlocks = 1u << 20;  // of k_tsdf_integrate: the stride loop takes the rest
static_assert(sizeof(TsdfIntegrateArgs) <= 320 && sizeof(TsdfRaycastArgs) <= 384, "the by-value arguments stay small");

// The tail of k_tsdf_raycast and of the two colour gathers: the block's lanes that say yes, counted into *count by ballot,
// through LDS, with one integer add per block.  Every thread of the block calls it.
__device__ __forceinline__ void tsdf_block_count(bool yes, int* count) {
  __shared__ int wave_counts[kTsdfBlockY];
  const int sum = __popcll(__ballot(yes));
  if (threadIdx.x == 0) wave_counts[threadIdx.y] = sum;
  __syncthreads();
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < kTsdfBlockY; ++w) total += wave_counts[w];
    if (total) reproject_add(count, total);
  }
}

// grid = (min(ceil(spans / 4), kTsdfMaxBlocks)), block = (64, 4); spans = ceil(nx / 64) * ny * nz
// (k_tsdf_integrate_color of pm_tsdf_color.hpp is this walk with a third counter: the two change together.)
__global__ void __launch_bounds__(kTsdfBlockX * kTsdfBlockY) k_tsdf_integrate(TsdfIntegrateArgs a) {
  __shared__ int wave_counts[kTsdfBlockY][2];
  const unsigned x_spans = ((unsigned)a.grid.nx + kTsdfLanes - 1) / kTsdfLanes;
  const unsigned long long spans = (unsigned long long)x_spans * (unsigned)a.grid.ny * (unsigned)a.grid.nz;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
  int in_view = 0, updated = 0;
  for (unsigned long long s = (unsigned long long)blockIdx.x * kTsdfBlockY + wave; s < spans;
       s += (unsigned long long)gridDim.x * kTsdfBlockY) {  // wave-uniform: nobody leaves in front of a ballot
    const unsigned long long row = s / x_spans;
    const int i = (int)((unsigned)(s - row * x_spans) * kTsdfLanes + threadIdx.x);
    const int k = (int)(row / (unsigned)a.grid.ny);
    const int j = (int)(row - (unsigned long long)k * (unsigned)a.grid.ny);
    const unsigned flags = i < a.grid.nx ? tsdf_integrate_lane(a, i, j, k) : 0u;
    in_view += __popcll(__ballot(flags & 1u));
    updated += __popcll(__ballot((flags >> 1) & 1u));
  }
  if (threadIdx.x == 0) wave_counts[threadIdx.y][0] = in_view, wave_counts[threadIdx.y][1] = updated;
  __syncthreads();
  if (threadIdx.x < 2 && threadIdx.y == 0) {  // lane c: counter c
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kTsdfBlockY; ++w) sum += wave_counts[w][threadIdx.x];
    if (sum) reproject_add(a.counts + threadIdx.x, sum);
  }
}

// grid = (ceil(cols / 64), ceil(rows / 4)), block = (64, 4)
__global__ void __launch_bounds__(kTsdfBlockX * kTsdfBlockY) k_tsdf_raycast(TsdfRaycastArgs a) {
  const int x = (int)(blockIdx.x * kTsdfLanes + threadIdx.x);
  const int y = (int)(blockIdx.y * kTsdfBlockY + threadIdx.y);
  const bool hit = x < a.cols && y < a.rows ? tsdf_ray_lane(a, x, y) : false;  // nobody leaves in front of the ballot
  tsdf_block_count(hit, a.counts);
}

}  // namespace pm
