// pm_fuse.hpp -- the kernels of pm_fuse_disparity (include/pm/imaging.h); included by pm_stages.hip alone.  The arithmetic
// and the per-thread bodies (fuse_splat_lane, fuse_lane) are pm_fuse_body.hpp's, the definition is tests/fuse_ref.py
// (DESIGN.md section 8c-8).
//
// Behind ONE memset of the four counts and, when filling, of the n splat maps behind them, two launches, neither of which
// waits for another workgroup:
//   k_fuse_splat     (only when filling) all n sources in one launch, the source in blockIdx.z: k_reproject_splat's shape and
//                    per-thread work (reproject_splat_lane) through the inverse motion into map blockIdx.z of the scratch, one
//                    integer atomicMax per surviving pixel;
//   k_fuse<RADIUS>   k_consistency's shape: a wavefront owns 256 consecutive pixels of a row, lane l takes pixels l, l + 64,
//                    l + 128, l + 192.  The point of a pixel is formed once; the loop over the sources is the outer, not
//                    unrolled one, its index is wave-uniform, so R, t and the pointers of a source come from the by-value
//                    argument with scalar loads; num, den, omin and omax of the four pixels stay in registers.  A pixel
//                    without a value reads the n splat words of its own position.  The four counts go by wavefront ballot,
//                    the four wavefronts meet in LDS, and ONE integer add per block and counter reaches memory.
// Only integer maximum and integer addition cross workgroups, so every output is a pure function of the inputs.  Every thread
// of a k_fuse block reaches every ballot and the barrier.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_fuse_body.hpp"

namespace pm {

// the launch shape (kFuseBlockX / Y, kFuseSpan) and kFuseCounters are pm_fuse_body.hpp's, where a CPU build reads them too
static_assert(kFuseBlockX == kFuseLanes, "threadIdx.y is the wavefront");
static_assert(sizeof(FuseArgs) <= 1088 && sizeof(FuseSplatArgs) <= 1024, "the by-value arguments stay near 1 KB");

// grid = (ceil(cols / 256), ceil(rows / 4), n), block = (64, 4)
__global__ void __launch_bounds__(kFuseBlockX * kFuseBlockY) k_fuse_splat(FuseSplatArgs a) {
  const int x = (int)(blockIdx.x * kFuseSpan + threadIdx.x);
  const int y = (int)(blockIdx.y * kFuseBlockY + threadIdx.y);
  if (x >= a.cols || y >= a.rows) return;
  fuse_splat_lane(a, (int)blockIdx.z, x, y);
}

// grid = (ceil(cols / 256), ceil(rows / 4)), block = (64, 4)
template <int RADIUS>
__global__ void __launch_bounds__(kFuseBlockX * kFuseBlockY) k_fuse(FuseArgs a) {
  __shared__ int wave_counts[kFuseBlockY][kFuseCounters];
  const int x = (int)(blockIdx.x * kFuseSpan + threadIdx.x);
  const int y = (int)(blockIdx.y * kFuseBlockY + threadIdx.y);
  const unsigned flags = x < a.cols && y < a.rows ? fuse_lane<RADIUS>(a, x, y) : 0u;  // nobody leaves in front of a ballot
#pragma unroll
  for (int c = 0; c < kFuseCounters; ++c) {  // threadIdx.y is the wavefront: the ballots are uniform in it
    int sum = 0;
#pragma unroll
    for (int k = 0; k < kFusePixelsPerLane; ++k) sum += __popcll(__ballot((flags >> (4 * c + k)) & 1u));
    if (threadIdx.x == 0) wave_counts[threadIdx.y][c] = sum;
  }
  __syncthreads();
  if (threadIdx.x < kFuseCounters && threadIdx.y == 0) {  // lane c: counter c
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kFuseBlockY; ++w) sum += wave_counts[w][threadIdx.x];
    if (sum) reproject_add(a.counts + threadIdx.x, sum);
  }
}

}  // namespace pm
