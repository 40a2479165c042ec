// pm_align.hpp -- the kernels of pm_align_evaluate (include/pm/imaging.h); included by pm_stages.hip alone.  The arithmetic and
// the per-thread bodies (align_lane, align_total) are pm_align_body.hpp's, the definition is tests/align_ref.py (DESIGN.md
// section 8c-12).
//
//   k_align_rows    (k_align_walk over align_lane) block (64, 4), one WAVEFRONT per row.  Lane l walks the pixels x = 64 c + l of its row and keeps its 28 lane
//                   sums in registers (56 VGPRs, binary64).  The camera, the motion and the options arrive by value and are
//                   wave-uniform: scalar registers.  The model map and its normals are coalesced loads; the new map is one gather
//                   per pixel behind every earlier test (align_pixel).  At the row's end each term's 64 lane sums meet in ONE
//                   balanced tree (wave_sum_f64) and lane 63 stores the 28 row sums.  The three counts go by ballot into
//                   registers, the four wavefronts meet in LDS, and ONE integer add per block and counter reaches memory
//                   (k_tsdf_raycast's tail).  The trip count is wave-uniform: every lane reaches every ballot and the barrier.
//   k_align_finish  one wavefront.  Lane e < 28 adds term e of the rows in ascending y and stores it into the record(s); lanes
//                   28 .. 31 copy the three counts and the zero pad beside them.
// No atomics on floating-point values, no cross-workgroup waits: the record is a pure function of the inputs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm/imaging.h"
#include "pm_align_body.hpp"

namespace pm {

static_assert(sizeof(AlignArgs) <= 256, "the by-value argument stays small");
static_assert(sizeof(pm_align_sums) == 240 && sizeof(pm_align_sums) == kAlignTerms * sizeof(double) + 4 * sizeof(int),
              "the record: 28 doubles in term order, then the counts and the pad");

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double v) {  // the two halves of a double through one DPP control; 0.0 where masked
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, ROW_MASK, 0xF, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, ROW_MASK, 0xF, false);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// The sum of v over the wavefront, in lane 63, in wave_sum_i32's sequence (pm_wave.hpp).  It IS the balanced binary tree
// s[i] = s[2i] + s[2i+1] of the definition bit for bit: step k adds to a lane's sum over its aligned group of 2^k lanes the sum
// over the group's sibling -- the two operands of the tree's node -- and binary64 addition is commutative, so it does not matter
// which sibling a lane sits in.  quad_perm [1,0,3,2]: pairs; quad_perm [2,3,0,1]: quads; row_half_mirror: lane i of an 8-group
// reads lane 7 - i, which sits in the other quad; row_mirror: the other 8-group of the 16-lane row; row_bcast15 adds lane 15 (row
// 0 / row 2) into rows 1 / 3; row_bcast31 adds lane 31 (rows 0 + 1) into rows 2 and 3: lane 63 ends with (r3 + r2) + (r1 + r0).
// Lanes outside a broadcast's row mask add +0.0 to a partial sum that nobody reads.
__device__ __forceinline__ double wave_sum_f64(double v) {
  v = v + dpp_f64<0xB1, 0xF>(v);
  v = v + dpp_f64<0x4E, 0xF>(v);
  v = v + dpp_f64<0x141, 0xF>(v);
  v = v + dpp_f64<0x140, 0xF>(v);
  v = v + dpp_f64<0x142, 0xA>(v);
  v = v + dpp_f64<0x143, 0xC>(v);
  return v;
}

// The row walk, stated once as a kernel template: k_align_rows below and k_align_photo_rows (pm_align_photo.hpp) are its two
// instances.  Lane()(a, x, y, acc) is one trip of one lane (align_lane): it adds the pixel's terms to acc and returns its class.
// grid = (ceil(rows / 4)), block = (64, 4)
template <typename Args, typename Lane>
__global__ void __launch_bounds__(kAlignBlockX * kAlignBlockY) k_align_walk(Args a) {
  __shared__ int wave_counts[kAlignBlockY][3];
  const int y = (int)(blockIdx.x * kAlignBlockY + threadIdx.y);
  const int chunks = y < a.rows ? align_chunks(a.cols) : 0;  // wave-uniform: nobody leaves in front of a ballot
  double acc[kAlignTerms];
#pragma unroll
  for (int k = 0; k < kAlignTerms; ++k) acc[k] = 0.0;
  int n_model = 0, n_gate = 0, n_used = 0;
#pragma unroll 1
  for (int c = 0; c < chunks; ++c) {
    const int x = c * kAlignLanes + (int)threadIdx.x;
    const int cls = x < a.cols ? Lane()(a, x, y, acc) : kAlignNoModel;  // beyond the row's end: +0.0 to every sum
    n_model += __popcll(__ballot(cls != kAlignNoModel));
    n_gate += __popcll(__ballot(cls >= kAlignGated));
    n_used += __popcll(__ballot(cls == kAlignUsed));
  }
#pragma unroll
  for (int k = 0; k < kAlignTerms; ++k) acc[k] = wave_sum_f64(acc[k]);
  if (threadIdx.x == kAlignLanes - 1 && y < a.rows) {
    double* out = a.row_sums + (size_t)y * kAlignTerms;
#pragma unroll
    for (int k = 0; k < kAlignTerms; ++k) out[k] = acc[k];
  }
  if (threadIdx.x == 0) wave_counts[threadIdx.y][0] = n_model, wave_counts[threadIdx.y][1] = n_gate, wave_counts[threadIdx.y][2] = n_used;
  __syncthreads();
  if (threadIdx.x < 3 && threadIdx.y == 0) {  // lane c: counter c
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kAlignBlockY; ++w) sum += wave_counts[w][threadIdx.x];
    if (sum) reproject_add(a.counts + threadIdx.x, sum);
  }
}

struct AlignLane {
  __device__ __forceinline__ int operator()(const AlignArgs& a, int x, int y, double* acc) const { return align_lane(a, x, y, acc); }
};
constexpr auto k_align_rows = &k_align_walk<AlignArgs, AlignLane>;

// grid = (1), block = (64).  `record` is the handle's; `also` the caller's d_sums, or null.
__global__ void __launch_bounds__(kAlignLanes) k_align_finish(const double* row_sums, int rows, const int* counts,
                                                              pm_align_sums* record, pm_align_sums* also) {
  const int e = (int)threadIdx.x;
  if (e < kAlignTerms) {
    const double sum = align_total(row_sums, rows, e);
    reinterpret_cast<double*>(record)[e] = sum;
    if (also) reinterpret_cast<double*>(also)[e] = sum;
  } else if (e < kAlignTerms + 4 && also) {  // the record's own counts are where k_align_rows added them
    const int c = e - kAlignTerms;
    (&also->n_model)[c] = c < 3 ? counts[c] : 0;
  }
}

}  // namespace pm
