// pm_align_photo.hpp -- the kernels of pm_bgr_luma and pm_align_photo_evaluate (include/pm/imaging.h); included by pm_stages.hip
// alone.  The arithmetic and the per-thread bodies (luma_lane, align_photo_lane) are pm_align_photo_body.hpp's, the definition is
// tests/align_photo_ref.py.
//
//   k_bgr_luma          block (64, 4), one pixel per lane: three loads (bytes or floats), one store.
//   k_align_photo_rows  pm_align.hpp's row walk (k_align_walk) over align_photo_lane: block (64, 4), one WAVEFRONT
//                       per row, 28 binary64 lane sums in registers, the arguments by value in scalar registers, wave_sum_f64's
//                       tree at the row's end, lane 63 storing the row sums, the three counts by ballot into one integer add per
//                       block and counter.  The model map and the model luma are coalesced loads; the new map and then the four
//                       taps are gathers behind every earlier test (align_photo_pixel).
// k_align_finish (pm_align.hpp) adds the rows as it is.  No atomics on floating-point values, no cross-workgroup waits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_align.hpp"
#include "pm_align_photo_body.hpp"

namespace pm {

static_assert(sizeof(AlignPhotoArgs) <= 256, "the by-value argument stays small");

// grid = (ceil(cols / 64), ceil(rows / 4)), block = (64, 4)
__global__ void __launch_bounds__(kAlignBlockX * kAlignBlockY) k_bgr_luma(LumaArgs a) {
  const int x = (int)(blockIdx.x * kAlignBlockX + threadIdx.x), y = (int)(blockIdx.y * kAlignBlockY + threadIdx.y);
  if (x < a.cols && y < a.rows) luma_lane(a, x, y);
}

struct AlignPhotoLane {
  __device__ __forceinline__ int operator()(const AlignPhotoArgs& a, int x, int y, double* acc) const {
    return align_photo_lane(a, x, y, acc);
  }
};
// grid = (ceil(rows / 4)), block = (64, 4)
constexpr auto k_align_photo_rows = &k_align_walk<AlignPhotoArgs, AlignPhotoLane>;

}  // namespace pm
