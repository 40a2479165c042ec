// pm_imaging_state.hpp -- what the two units behind include/pm/imaging.h share: pm_imaging.hip (the imaging rows and the
// device-buffer helpers) and pm_stages.hip (the stages that read a finished disparity map).  One state object per handle,
// in the handle's one opaque slot (pm_internal.hpp), created on first use by either unit and released by
// pm_internal::release_imaging (pm_imaging.hip).  Host only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>

#include "pm_devbuf.hpp"
#include "pm_hipres.hpp"
#include "pm_internal.hpp"

namespace pm {

// Device state of the imaging entry points, created on first use and released by pm_destroy.  The scratch buffers grow
// to the largest size asked for (DevBuf::reserve).
struct ImagingState {
  // ---- pm_imaging.hip ----
  DevBuf<unsigned> img_scalars;  // device: [0] max range / min disparity bits, [1] dark-pixel count, [2..3] V min / max
  // stereo-ready enhancement: row-pass output, bgr / illuminant, Gaussian taps
  DevBuf<float> enh_tmp;
  DevBuf<float> enh_q;
  DevBuf<float> enh_taps;
  int enh_ksize = 0;  // what enh_taps holds
  double enh_sigma = 0;
  // pm_match_bgr_device: blurred illuminants of n pairs (left, right) and their value min / max words
  DevBuf<float> bgr_blur;
  DevBuf<unsigned> bgr_mm;
  // fast guided filter: binary64 row sums, a / b planes, interleaved mean_a / mean_b of the coarse image (one allocation)
  DevBuf<char> gf_buf;
  // pm_gather_pixels: [bad flag, pad][n x channels floats][n x 2 coordinates]
  DevBuf<char> gat_buf;
  // pm_match_raw_device: the rectified pairs, [left, right][n][rows][cols] bytes; pm_match_raw_bgr_device: the rectified
  // BGR images the caller did not ask for, [n][rows][cols][3] bytes each
  DevBuf<uint8_t> rect_buf;
  // ---- pm_stages.hip (kCountsHeader: the counts of a call, padded to 16 bytes) ----
  // pm_point_cloud: [0] the count, [1 ..] one word per block of kCloudBlock items: its count, then its offset
  DevBuf<int> cloud_blocks;
  // pm_filter_speckles: [0] the removed count (kCountsHeader words, cleared per call), then the working labels and the
  // root sizes, one word per pixel each
  DevBuf<int> speckle_buf;
  // pm_grid_mesh: [0] the vertex count, [1] the triangle count, then one word per block of kMeshBlock items for each of
  // the two (its count, then its offset), then the organised slot map, one word per grid item
  DevBuf<int> mesh_buf;
  // pm_reproject_disparity: kCountsHeader words ([0], [1]: the counts), the left and the right splat map, one word per
  // pixel each (the memset of a call clears up to here), then the closed left seed of a call without d_seed_l
  DevBuf<unsigned> reproject_buf;
  // pm_filter_consistency: kCountsHeader words ([0] valid pixels, [1] kept pixels), cleared per call
  DevBuf<int> consistency_counts;
  // pm_disparity_confidence: kCountsHeader words ([0] valid, [1] measured, [2] kept pixels; cleared per call), then the
  // right image's gradient (one float per pixel), then the left image's saturated gradient (one byte per pixel)
  DevBuf<int> confidence_buf;
  // pm_fuse_disparity: kCountsHeader words ([0] valid, [1] kept, [2] fused, [3] filled pixels), then, for a call that fills,
  // one splat map of one word per pixel for each source; the memset of a call clears all of it
  DevBuf<unsigned> fuse_buf;
  // pm_track_features / pm_estimate_motion: kCountsHeader words ([0] the number of features), one word per cell (its feature's
  // pixel index or -1), one word per cell (the feature list) and, for pm_estimate_motion, one pm_track per cell
  DevBuf<int> track_buf;
  // pm_tsdf_integrate / pm_tsdf_raycast: kCountsHeader words ([0], [1]: the counts of the call), cleared per call
  DevBuf<int> tsdf_counts;
  // pm_tsdf_mesh: kCountsHeader words ([0] the vertex count, [1] the triangle count), one word per group of 1024 spans and one
  // per 64-node span of a row, for the vertices and for the triangles each (its count, then its offset), one word per node (its vertex mask and its rank in
  // the span), one byte per node (its crossing edges and whether its cell is live)
  DevBuf<int> tsdf_mesh_buf;
  // pm_align_evaluate / pm_align_disparity: a 256-byte slot for the record (pm_align_sums; its counts are where the launch adds
  // them, cleared per call), then one row sum of 28 doubles per row; and the page-locked record the downloads land in
  DevBuf<char> align_buf;
  HostBuf align_host;
  // pm_align_photo_evaluate / pm_align_color_disparity: a second 256-byte record slot and a second run of row sums, then the two
  // luma planes of pm_align_color_disparity (the model's, the new image's), one float per pixel each; and the page-locked
  // record the photometric downloads land in
  DevBuf<char> align_photo_buf;
  HostBuf align_photo_host;
};

#define PM_HIP(h, call)                                                                                     \
  do {                                                                                                      \
    hipError_t e_ = (call);                                                                                 \
    if (e_ != hipSuccess) {                                                                                 \
      pm_internal::set_error((h), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return PM_ERR_HIP;                                                                                    \
    }                                                                                                       \
  } while (0)

#define set_err pm_internal::set_error

static inline int launch_check(pm_handle* h, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_err(h, "launch of %s failed: %s", what, hipGetErrorString(e));
    return PM_ERR_HIP;
  }
  return PM_OK;
}

// null: out of host memory
static inline ImagingState* state_of(pm_handle* h) {
  void** slot = pm_internal::imaging_slot(h);
  if (!*slot) *slot = new (std::nothrow) ImagingState();
  return static_cast<ImagingState*>(*slot);
}

}  // namespace pm
