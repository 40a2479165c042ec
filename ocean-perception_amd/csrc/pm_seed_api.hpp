// pm_seed_api.hpp -- what the engine sees of the device seeder (pm_seed.hpp holds the kernels, pm_seed.hip is their
// translation unit): parameters, the scratch a handle owns (released with it), and the enqueue-only entry points.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pm_devbuf.hpp"
#include "pm_seed_plan.hpp"  // SeedParams, kSeedMaxFeatures, plan_seed

namespace pm {

constexpr int kSubpixMaxWin = 15;       // largest half window of cornerSubPix the scratch is sized for
constexpr int kSubpixMatchWin = 10;     // StereoMatcher's fixed window (stereo_matcher.cpp:97)

constexpr int kSeedCounters = 8;        // SeedScratch::counters
constexpr int kSeedCapExtra = 64;       // candidate slots beyond one per pixel (SeedScratch::cap; no plane slack)
constexpr int kSubpixMaskStride = 1024;  // floats between the two masks of SeedScratch::sp_mask (31 * 31 = 961)

// Scratch owned by the handle (sized for max_rows x max_cols).
struct SeedScratch {
  DevBuf<float> eig;                 // [rows][pitch]
  DevBuf<unsigned long long> keys;   // [cap] candidates, then sorted
  DevBuf<unsigned long long> keys_sorted;
  DevBuf<unsigned> counters;         // [kSeedCounters]: [0] = max response bits, [1] = candidate count, [2] = accepted
                                     // count, [3] = grid overflow flag
  DevBuf<int> kp_xy;                 // [kSeedMaxFeatures][2]
  DevBuf<float> kp_d;                // [kSeedMaxFeatures] matched disparity of a corner, < 0 = no match
  DevBuf<float> kp_f;                // [kSeedMaxFeatures][2] sub-pixel corner positions (subpixel_corners)
  // only for handles that ask for cornerSubPix (seed_subpix_prepare):
  DevBuf<float> sp_buf;              // neighbourhoods, [(2 * kSubpixMaxWin + 3)^2][kSeedMaxFeatures]
  DevBuf<float> sp_mask;             // window masks: detector's [(2 w + 1)^2] at 0, matcher's [21 * 21] at kSubpixMaskStride
  int sp_mask_win = 0, sp_mask_zero = 0;  // what the detector's mask was built for
  DevBuf<void> sort_tmp;
  size_t sort_tmp_bytes = 0;         // what hipcub asked for (it takes the size as an argument)
  int cap = 0;
  // the selection kernels leave counters[0], [1] and [3] at zero for the next map; false after an allocation or an
  // enqueue that did not get as far as the selection: the next map then starts with a memset
  mutable bool counters_clean = false;
};

// Allocates the scratch for planes of `plane_elems` pixels (rows x pitch of the plan).  Every pixel can be a candidate:
// the 3x3 test is not strict, so plateaus of EQUAL responses (periodic images) pass whole; a capacity of a quarter of the
// pixels dropped candidates there in whatever order the atomics fell.
hipError_t seed_scratch_alloc(SeedScratch& sc, size_t plane_elems, hipStream_t stream);
// the masks and the neighbourhood buffer of cv::cornerSubPix, for handles whose parameters ask for it (synchronises
// the stream when it has to upload the masks: call outside captures)
hipError_t seed_subpix_prepare(SeedScratch& sc, const SeedParams& sp, hipStream_t stream);

// cv::cornerSubPix with the detector's window parameters of `sp` on n device points (needs seed_subpix_prepare)
hipError_t seed_corner_subpix(const SeedScratch& sc, const SeedParams& sp, const uint8_t* img, int rows, int cols, int pitch,
                              float* d_xs, float* d_ys, int n, hipStream_t stream);
// The launch sequence of one map comes in kSeedStages parts (bit i of `stages` = part i; all by default).  Parts of one
// map go onto one stream in order; a caller with several maps on several streams may interleave them part by part.
constexpr int kSeedStages = 5;
constexpr unsigned kSeedAllStages = (1u << kSeedStages) - 1u;
// `out`: a row-major map with out_pitch elements per row, or -- out_pitch < 0 -- one of the engine's state planes (four
// rows interleaved, pm_device.hpp::state_at, pitch -out_pitch).
// PatchmatchGpu::SparseInit(iml, imr, f)  (patchmatch_gpu.cu:414-442): dilation half-width 2^f + 1, map at image size
// forced_route (pm_seed_plan.hpp::SeedRoute; the test hooks): the selection route instead of the plan's own choice;
// hipErrorInvalidValue where the plan refuses it.
hipError_t seed_sparse_init(const SeedScratch& sc, const SeedParams& sp, const uint8_t* left, const uint8_t* right,
                            int rows, int cols, int pitch, int dilate_factor, float* out, int out_pitch,
                            hipStream_t stream, unsigned stages = kSeedAllStages, int forced_route = kSeedRouteAuto);
// Patchmatch::Initialize(iml, imr, f)  (patchmatch.cpp:60-84): half-width 2^(f-1) + 1, map of size / f, scaled by 2^-f;
// downsample_factor >= 1
hipError_t seed_initialize(const SeedScratch& sc, const SeedParams& sp, const uint8_t* left, const uint8_t* right,
                           int rows, int cols, int pitch, int downsample_factor, float* out, int out_pitch,
                           hipStream_t stream, unsigned stages = kSeedAllStages);

// ---- single launches of the sequence on the scratch as the caller filled it (the test hooks of include/pm/testing.h)
// k_seed_match alone on the n <= kSeedMaxFeatures corners in sc.kp_xy (use_kp_f: with their sub-pixel positions in
// sc.kp_f); counters[2] must hold n.  Results in sc.kp_d.
hipError_t seed_match_corners(const SeedScratch& sc, const SeedParams& sp, const uint8_t* left, const uint8_t* right,
                              int rows, int cols, int pitch, int n, bool use_kp_f, hipStream_t stream);
// The memset, k_seed_splat and -- where out_rows x out_cols differs from rows x cols -- k_seed_resize_nearest on the
// n <= kSeedMaxFeatures corners in sc.kp_xy / sc.kp_d; counters[2] must hold n.  `pitch`: of the full-size plane a
// resize starts from (sc.eig).
hipError_t seed_splat_corners(const SeedScratch& sc, int n, int rows, int cols, int pitch, int k, float inv_scale,
                              int dedup, int out_rows, int out_cols, float* out, int out_pitch, hipStream_t stream);

}  // namespace pm
