// pm_consistency.hpp -- the kernel of pm_filter_consistency (include/pm/imaging.h); included by pm_stages.hip alone.  The
// arithmetic and the per-thread body (consistency_lane) are pm_consistency_body.hpp's, the definition is
// tests/consistency_ref.py.
//
// Behind ONE 16-byte memset of the two counts, one launch that waits for no other workgroup:
//   k_consistency<RADIUS>  a wavefront owns 256 consecutive pixels of a row, 64 at a time: lane l takes pixels l, l + 64,
//                          l + 128, l + 192 (k_reproject_splat's shape: four loads in flight, four independent binary64
//                          chains per lane).  The point of a pixel is formed once; the loop over the sources is the outer,
//                          not unrolled one, its index is wave-uniform, so R, t and the map pointer of a source come from
//                          the by-value argument with scalar loads; the window loops are unrolled per RADIUS.  Every lookup is
//                          a gather (an inverse warp): no atomic touches a map.  Valid and kept pixels are counted by
//                          wavefront ballot, the four wavefronts meet in LDS, and ONE integer add per block and counter
//                          reaches memory.
// Only integer addition crosses workgroups, so every output is a pure function of the inputs.  Every thread of a block
// reaches every ballot and the barrier.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_consistency_body.hpp"

namespace pm {

// the launch shape (kConsistencyBlockX / Y, kConsistencySpan) is pm_consistency_body.hpp's, where a CPU build reads it too
static_assert(kConsistencyBlockX == kConsistencyLanes, "threadIdx.y is the wavefront");
static_assert(sizeof(ConsistencyArgs) <= 1024, "the by-value argument stays under 1 KB");

// grid = (ceil(cols / 256), ceil(rows / 4)), block = (64, 4)
template <int RADIUS>
__global__ void __launch_bounds__(kConsistencyBlockX * kConsistencyBlockY) k_consistency(ConsistencyArgs a) {
  __shared__ int wave_counts[kConsistencyBlockY][2];
  const int x = (int)(blockIdx.x * kConsistencySpan + threadIdx.x);
  const int y = (int)(blockIdx.y * kConsistencyBlockY + threadIdx.y);
  const unsigned flags = x < a.cols && y < a.rows ? consistency_lane<RADIUS>(a, x, y) : 0u;  // nobody leaves in front of a ballot
  int valid = 0, kept = 0;
#pragma unroll
  for (int k = 0; k < kConsistencyPixelsPerLane; ++k) {  // threadIdx.y is the wavefront: the ballots are uniform in it
    valid += __popcll(__ballot((flags >> k) & 1u));
    kept += __popcll(__ballot((flags >> (4 + k)) & 1u));
  }
  if (threadIdx.x == 0) {
    wave_counts[threadIdx.y][0] = valid;
    wave_counts[threadIdx.y][1] = kept;
  }
  __syncthreads();
  if (threadIdx.x < 2 && threadIdx.y == 0) {  // lane 0: valid, lane 1: kept
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kConsistencyBlockY; ++w) sum += wave_counts[w][threadIdx.x];
    if (sum) reproject_add(a.counts + threadIdx.x, sum);
  }
}

}  // namespace pm
