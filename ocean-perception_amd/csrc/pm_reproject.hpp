// pm_reproject.hpp -- the kernels of pm_reproject_disparity (include/pm/imaging.h); included by pm_stages.hip alone.  The
// arithmetic and the per-thread bodies (reproject_splat_lane, reproject_right_lane, reproject_stage_cell,
// reproject_finish_pixel) are pm_reproject_body.hpp's, the definition is tests/reproject_ref.py.
//
// Behind ONE memset that zeroes both splat maps and the two counts, four launches, none of which waits for another workgroup:
//   k_reproject_splat        a wavefront owns 256 consecutive source pixels of a row, 64 at a time: lane l takes pixels
//                            l, l + 64, l + 128, l + 192, carries each through the motion and raises the word it lands on
//                            with one integer atomicMax, so that a wavefront's atomics fall on near-consecutive words;
//   k_reproject_finish       a block of 64 x 4 threads owns a tile of 64 x 16 pixels: it stages the tile and an r-wide halo in
//                            LDS, closes (a pixel that was hit is copied, a hole takes the maximum of its window), stores, and
//                            counts the pixels > 0 by wavefront ballot; ONE integer add per block reaches the count;
//   k_reproject_splat_right  reads the closed left seed in the same layout and raises word (y, rint(x - s));
//   k_reproject_finish       again, on the right view.
// Only integer maximum and integer addition cross workgroups: both are associative and commutative, so the result does not
// depend on the order of arrival.  Every thread of a finish block reaches every barrier and ballot.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_reproject_body.hpp"

namespace pm {

// the launch shapes (kReprojectBlockX / Y, kReprojectSpan) are pm_reproject_body.hpp's, where a CPU build reads them too
static_assert(kReprojectBlockX == kReprojectTileW && kReprojectTileH % kReprojectBlockY == 0, "a wavefront per tile row");
static_assert(kReprojectBlockX == kReprojectLanes, "threadIdx.y is the wavefront");

// grid = (ceil(cols / 256), ceil(rows / 4)), block = (64, 4)
__global__ void __launch_bounds__(kReprojectBlockX * kReprojectBlockY) k_reproject_splat(ReprojectArgs a) {
  const int x = (int)(blockIdx.x * kReprojectSpan + threadIdx.x);
  const int y = (int)(blockIdx.y * kReprojectBlockY + threadIdx.y);
  if (x >= a.cols || y >= a.rows) return;
  reproject_splat_lane(a, x, y);
}

// grid and block as k_reproject_splat
__global__ void __launch_bounds__(kReprojectBlockX * kReprojectBlockY) k_reproject_splat_right(ReprojectRightArgs a) {
  const int x = (int)(blockIdx.x * kReprojectSpan + threadIdx.x);
  const int y = (int)(blockIdx.y * kReprojectBlockY + threadIdx.y);
  if (x >= a.cols || y >= a.rows) return;
  reproject_right_lane(a, x, y);
}

// grid = (ceil(cols / 64), ceil(rows / 16)), block = (64, 4).  Runs for r = 0 too: copy + count.
__global__ void __launch_bounds__(kReprojectBlockX * kReprojectBlockY) k_reproject_finish(ReprojectFinishArgs a) {
  __shared__ unsigned tile[kReprojectTileWords];
  __shared__ int wave_count[kReprojectBlockY];
  const int x0 = (int)blockIdx.x * kReprojectTileW, y0 = (int)blockIdx.y * kReprojectTileH;
  const int tid = (int)(threadIdx.y * kReprojectBlockX + threadIdx.x);
  const int w = kReprojectTileW + 2 * a.r, hgt = kReprojectTileH + 2 * a.r;
  for (int ly = (int)threadIdx.y; ly < hgt; ly += kReprojectBlockY)  // a wavefront per staged row: coalesced, no division
    for (int lx = (int)threadIdx.x; lx < w; lx += kReprojectBlockX) reproject_stage_cell(a, tile, lx, ly, x0, y0);
  __syncthreads();
  int mine = 0;
#pragma unroll
  for (int k = 0; k < kReprojectTileH / kReprojectBlockY; ++k) {
    const bool set = reproject_finish_pixel(a, tile, x0, y0, (int)threadIdx.x, (int)threadIdx.y + k * kReprojectBlockY);
    mine += __popcll(__ballot(set));  // threadIdx.y is the wavefront: the ballot is uniform in it
  }
  if (threadIdx.x == 0) wave_count[threadIdx.y] = mine;
  __syncthreads();
  if (tid == 0) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kReprojectBlockY; ++w) sum += wave_count[w];
    if (sum) reproject_add(a.count, sum);
  }
}

}  // namespace pm
