// pm_confidence.hpp -- the kernels of pm_disparity_confidence (include/pm/imaging.h); included by pm_stages.hip alone.  The
// arithmetic and the per-thread steps are pm_confidence_body.hpp's, the definition is tests/confidence_ref.py (DESIGN.md
// section 8c-7).
//
// Behind ONE 16-byte memset of the three counts, two launches:
//   k_confidence_grad       the Sobel magnitudes of the caller's two raw images (sobel_mag of pm_device.hpp, k_prep's own):
//                           the left one saturated to a byte -- all a window reads of its own image -- the right one as f32.
//   k_confidence<PW, PH>    one workgroup per 32x8 pixel tile, one pixel per thread (k_noise_cost_tiled's shape).  Every
//                           pixel evaluates the functor four times: at d, at d - 1 and d + 1 (bilinear target lerp) and at 0
//                           (a plain byte SAD, v_sad_u8).  The reference window tile and the target rows are staged in LDS
//                           ONCE for all four: the target tile spans the columns from the tile's smallest ipx (of d + 1) to
//                           behind the reference window (cost(0) needs those).  Where the three lerped windows are one
//                           column apart with one fraction -- the usual case -- ONE pass over pw + 2 lerped columns per row
//                           serves all three (confidence_cost3); the byte SAD rides on the reference bytes of the pass
//                           that forms cost(d).  A tile whose span exceeds kConfTileRW columns evaluates
//                           from global memory with the same arithmetic.  PW = PH = 0: the window comes from the argument.
//                           Outputs are plain vector stores; valid, measured and kept pixels are counted by wavefront
//                           ballot, the four wavefronts meet in LDS and ONE integer add instruction per block reaches memory.
// Only integer addition crosses workgroups, so every output is a pure function of the inputs.  Every thread of a block
// reaches every barrier and every ballot.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_confidence_body.hpp"

namespace pm {

constexpr int kConfGradBlockX = 64, kConfGradBlockY = 4;  // the rows of a grid stay within pm_backproject's bound

// grid = (ceil(cols / 64), ceil(rows / 4)), block = (64, 4)
__global__ void __launch_bounds__(kConfGradBlockX * kConfGradBlockY) k_confidence_grad(const uint8_t* __restrict__ left,
                                                                                       const uint8_t* __restrict__ right,
                                                                                       int rows, int cols,
                                                                                       uint8_t* __restrict__ gl8,
                                                                                       float* __restrict__ gr) {
  const int x = (int)(blockIdx.x * kConfGradBlockX + threadIdx.x), y = (int)(blockIdx.y * kConfGradBlockY + threadIdx.y);
  if (x >= cols || y >= rows) return;
  const size_t o = (size_t)y * cols + x;
  gl8[o] = (uint8_t)sat_u8(sobel_mag(left, (size_t)cols, rows, cols, x, y));
  gr[o] = sobel_mag(right, (size_t)cols, rows, cols, x, y);
}

// grid = (ceil(cols / 32), ceil(rows / 8)), block = 256
template <int PW, int PH>
__global__ void __launch_bounds__(kConfThreads) k_confidence(ConfidenceArgs a) {
  constexpr int MW = PW ? PW : PM_MAX_PATCH, MH = PH ? PH : PM_MAX_PATCH;
  constexpr int TR = kConfTileH + MH - 1, LWP = (kConfTileW + MW - 1 + 3) & ~3;
  __shared__ __attribute__((aligned(16))) float s_rg[TR * kConfTileRW];
  __shared__ __attribute__((aligned(4))) uint8_t s_r8[TR * kConfTileRW];
  __shared__ __attribute__((aligned(4))) uint8_t s_rg8[TR * kConfTileRW];
  __shared__ __attribute__((aligned(4))) uint8_t s_l8[TR * LWP];
  __shared__ __attribute__((aligned(4))) uint8_t s_lg[TR * LWP];
  __shared__ int s_red[4][2];
  __shared__ int s_counts[4][3];

  const int tid = (int)threadIdx.x, tx = tid & (kConfTileW - 1), ty = tid / kConfTileW;
  const int x0 = (int)blockIdx.x * kConfTileW, y0 = (int)blockIdx.y * kConfTileH;
  const int x = x0 + tx, y = y0 + ty;
  const ConfidenceLane l = confidence_lane_setup(a, x, y);

  // column range of the target tile: min / max over the block's measured lanes
  int lo = l.measured ? l.lo : 0x7fffffff, hi = l.measured ? l.hi : -0x7fffffff;
#pragma unroll
  for (int ofs = 32; ofs > 0; ofs >>= 1) {
    lo = min(lo, __shfl_xor(lo, ofs, 64));
    hi = max(hi, __shfl_xor(hi, ofs, 64));
  }
  if ((tid & 63) == 0) {
    s_red[tid >> 6][0] = lo;
    s_red[tid >> 6][1] = hi;
  }
  __syncthreads();
  lo = min(min(s_red[0][0], s_red[1][0]), min(s_red[2][0], s_red[3][0]));
  hi = max(max(s_red[0][1], s_red[1][1]), max(s_red[2][1], s_red[3][1]));

  ConfidenceTile t = {s_l8, s_lg, s_r8, s_rg8, s_rg, LWP, 0, 0};
  const bool any = hi >= lo;                                                // uniform: somebody is measured
  const bool tiled = any && confidence_tile_plan(lo, hi, a.pw, &t.lo4, &t.rw);  // uniform
  if (tiled) confidence_fill(a, t, x0, y0, tid);
  __syncthreads();
  unsigned bits;
  if (tiled)
    bits = confidence_lane_finish<PW, PH>(a, l, ConfidenceTileSrc{t, tx, ty}, x, y);
  else
    bits = confidence_lane_finish<PW, PH>(a, l, ConfidenceGlobalSrc{a, x, y}, x, y);

  // threadIdx.x >> 6 is the wavefront: the ballots are uniform in it
  const int valid = __popcll(__ballot(bits & 1u)), measured = __popcll(__ballot(bits & 2u)), kept = __popcll(__ballot(bits & 4u));
  if ((tid & 63) == 0) {
    s_counts[tid >> 6][0] = valid;
    s_counts[tid >> 6][1] = measured;
    s_counts[tid >> 6][2] = kept;
  }
  __syncthreads();
  if (tid < 3) {  // lane 0: valid, lane 1: measured, lane 2: kept
    const int sum = s_counts[0][tid] + s_counts[1][tid] + s_counts[2][tid] + s_counts[3][tid];
    if (sum) reproject_add(a.counts + tid, sum);
  }
}

}  // namespace pm
