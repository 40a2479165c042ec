// pm_internal.hpp -- what the other translation units of libvehicle_pm_gpu.so may use of a pm_handle
// (defined in pm_engine.hip).  Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include "pm/patchmatch.h"

namespace pm {
struct BgrSource;
struct CloudCam;
}

namespace pm_internal __attribute__((visibility("hidden"))) {
int device(const pm_handle* h);
hipStream_t stream(pm_handle* h);
const pm_params& params(const pm_handle* h);
void plan_size(const pm_handle* h, int* max_rows, int* max_cols);
void set_error(pm_handle* h, const char* fmt, ...);
void** imaging_slot(pm_handle* h);     // storage for pm_imaging_state.hpp's state
// pm_match_bgr_device behind its own checks: pm_match_device (its refusals and error texts included) on n pairs whose prep
// stage reads `src` (pm_kernels.hpp::k_prep_bgr) instead of 8-bit gray images
int match_bgr(pm_handle* h, int n, const pm::BgrSource& src, int rows, int cols, const float* d_seed_l,
              const float* d_seed_r, float* d_disp_l, float* d_disp_r);
void release_imaging(pm_handle* h);    // defined in pm_imaging.hip, called by pm_destroy
// pm_planes_normals behind its argument checks (defined in pm_planes_host.hip, the unit of the plane-mode kernels):
// PM_ERR_STATE unless the handle is in PM_MODE_PLANES and holds the state of pair `pair` at rows x cols
int planes_normals(pm_handle* h, int pair, const pm::CloudCam& cam, const float* d_disp_l, int rows, int cols,
                   float* d_normals);
}  // namespace pm_internal
