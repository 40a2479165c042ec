// pm_stages.hip -- C-ABI implementation of the stages of include/pm/imaging.h that read a finished disparity map: points,
// plane-mode normals and the compacted cloud, the windowed plane fit, the speckle filter, the grid mesh, the temporal
// seeds, the consistency filter, the matching confidence, the sequence fusion, the TSDF volume with its mesh, the feature
// tracks of the motion estimate and the dense alignment of a map against a model.  Like pm_imaging.hip it reaches the handle only through pm_internal.hpp, and it shares that unit's one
// state object (pm_imaging_state.hpp).  Every entry point: its argument checks in a fixed order (the first fault is the one
// reported), then the device, then its launches on the handle's stream.
#include "pm/imaging.h"
#include "pm/testing.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <new>
#include <vector>

#include "pm_align.hpp"
#include "pm_align_photo.hpp"
#include "pm_cloud.hpp"
#include "pm_confidence.hpp"
#include "pm_consistency.hpp"
#include "pm_fuse.hpp"
#include "pm_imaging_state.hpp"
#include "pm_mesh.hpp"
#include "pm_normals_fit.hpp"
#include "pm_reproject.hpp"
#include "pm_speckle.hpp"
#include "pm_track.hpp"
#include "pm_tsdf.hpp"
#include "pm_tsdf_color.hpp"
#include "pm_tsdf_mesh.hpp"
#include "pm_tune.hpp"

using namespace pm;

// ---- what the stages share --------------------------------------------------------------------------------------------
namespace {

// The first null pointer of a list, by its name.
struct NamedPointer {
  const char* name;
  const void* p;
};

int check_not_null(pm_handle* h, const char* what, std::initializer_list<NamedPointer> pointers) {
  for (const NamedPointer& q : pointers)
    if (!q.p) {
      set_err(h, "%s: null %s", what, q.name);
      return PM_ERR_INVALID_ARG;
    }
  return PM_OK;
}

// A call with every output null; `names` as the message lists them, `parenthesised` the form of the older stages.
int check_any_output(pm_handle* h, const char* what, std::initializer_list<const void*> outputs, const char* names,
                     bool parenthesised = false) {
  for (const void* p : outputs)
    if (p) return PM_OK;
  set_err(h, parenthesised ? "%s: no output (%s are all null)" : "%s: no output: %s are all null", what, names);
  return PM_ERR_INVALID_ARG;
}

int check_cloud_camera(pm_handle* h, const char* what, const pm_cloud_camera* cam) {
  if (int rc = check_not_null(h, what, {{"camera", cam}})) return rc;
  static const char* const names[5] = {"fx", "fy", "cx", "cy", "baseline"};
  const double* e = reinterpret_cast<const double*>(cam);
  static_assert(sizeof(pm_cloud_camera) == 5 * sizeof(double), "pm_cloud_camera is 5 doubles");
  for (int i = 0; i < 5; ++i)
    if (!std::isfinite(e[i])) {
      set_err(h, "%s: %s of the camera is not finite", what, names[i]);
      return PM_ERR_INVALID_ARG;
    }
  if (cam->fx == 0.0 || cam->fy == 0.0) {
    set_err(h, "%s: fx / fy of the camera must not be 0", what);
    return PM_ERR_INVALID_ARG;
  }
  return PM_OK;
}

int check_cloud_shape(pm_handle* h, const char* what, int rows, int cols) {
  if (rows < 1 || cols < 1) {
    set_err(h, "%s: empty image (%dx%d)", what, cols, rows);
    return PM_ERR_INVALID_ARG;
  }
  if ((long long)rows * cols > INT32_MAX || (rows + kCloudBlockY - 1) / kCloudBlockY > 65535) {
    set_err(h, "%s: %dx%d pixels exceed a 32-bit pixel index or the launch grid", what, cols, rows);
    return PM_ERR_SIZE;
  }
  return PM_OK;
}

// the cloud and the mesh; `filter` is not null
int check_cloud_filter(pm_handle* h, const char* what, const pm_cloud_filter* filter) {
  if (filter->stride < 1) {
    set_err(h, "%s: stride %d must be >= 1", what, filter->stride);
    return PM_ERR_INVALID_ARG;
  }
  if (std::isnan(filter->min_disp) || !(filter->max_range >= 0.f)) {
    set_err(h, "%s: min_disp must not be NaN and max_range must be >= 0 (0 = no limit)", what);
    return PM_ERR_INVALID_ARG;
  }
  return PM_OK;
}

// the normals fit, the speckle filter and the mesh
int check_max_diff(pm_handle* h, const char* what, float max_diff) {
  if (!std::isfinite(max_diff) || max_diff < 0.f) {
    set_err(h, "%s: max_diff must be finite and >= 0", what);
    return PM_ERR_INVALID_ARG;
  }
  return PM_OK;
}

// the seeds and the tracks
int check_disp_limits(pm_handle* h, const char* what, float min_disp, float max_disp) {
  if (!(min_disp >= 0.f) || !(max_disp >= 0.f)) {
    set_err(h, "%s: %s must be >= 0 and not NaN%s", what, !(min_disp >= 0.f) ? "min_disp" : "max_disp",
            !(min_disp >= 0.f) ? "" : " (0 = no limit)");
    return PM_ERR_INVALID_ARG;
  }
  return PM_OK;
}

// `whose`: the motion as the message names it ("the motion", "motions[1]", "the pose", "the guess")
int check_motion(pm_handle* h, const char* what, const pm_motion& m, const char* whose) {
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(i < 9 ? m.R[i] : m.t[i - 9])) {
      set_err(h, "%s: %s[%d] of %s is not finite", what, i < 9 ? "R" : "t", i < 9 ? i : i - 9, whose);
      return PM_ERR_INVALID_ARG;
    }
  return PM_OK;
}

// the consistency filter and the fusion: the earlier maps of the sequence with their motions ...
static_assert(kFuseMaxSources == kConsistencyMaxSources && kFuseMaxRadius == kConsistencyMaxRadius, "one set of limits");

int check_sources(pm_handle* h, const char* what, int n_sources, const float* const* d_sources, const pm_motion* motions) {
  if (n_sources < 1 || n_sources > kConsistencyMaxSources) {
    set_err(h, "%s: n_sources %d outside 1..%d", what, n_sources, kConsistencyMaxSources);
    return PM_ERR_INVALID_ARG;
  }
  for (int k = 0; k < n_sources; ++k) {
    if (!d_sources[k]) {
      set_err(h, "%s: null d_sources[%d]", what, k);
      return PM_ERR_INVALID_ARG;
    }
    char whose[24];
    std::snprintf(whose, sizeof whose, "motions[%d]", k);
    if (int rc = check_motion(h, what, motions[k], whose)) return rc;
  }
  return PM_OK;
}

// ... and the options of the vote
int check_votes(pm_handle* h, const char* what, float max_diff, int radius, int min_consistent, int max_conflicts,
                int n_sources) {
  if (int rc = check_max_diff(h, what, max_diff)) return rc;
  if (radius < 0 || radius > kConsistencyMaxRadius) {
    set_err(h, "%s: radius %d outside 0..%d", what, radius, kConsistencyMaxRadius);
    return PM_ERR_INVALID_ARG;
  }
  if (min_consistent < 0 || min_consistent > n_sources) {
    set_err(h, "%s: min_consistent %d outside 0..n_sources (%d)", what, min_consistent, n_sources);
    return PM_ERR_INVALID_ARG;
  }
  if (max_conflicts < 0 || max_conflicts > kConsistencyMaxSources) {
    set_err(h, "%s: max_conflicts %d outside 0..%d", what, max_conflicts, kConsistencyMaxSources);
    return PM_ERR_INVALID_ARG;
  }
  return PM_OK;
}

// A motion into the arrays of a kernel's arguments; null is the identity, and `t` may be null where only R is wanted.
void set_motion(double R[9], double t[3], const pm_motion* m) {
  for (int i = 0; i < 9; ++i) R[i] = m ? m->R[i] : (i % 4 == 0 ? 1.0 : 0.0);
  for (int i = 0; t && i < 3; ++i) t[i] = m ? m->t[i] : 0.0;
}

// The grid of the three launches that give a block 256 pixels of a row and four rows (the seeds' splats, the consistency
// filter, the fusion): pm_reproject_body.hpp states it once, and the other two stages' constants are aliases of it.
dim3 span_grid(int rows, int cols) {
  const SpanBlocks blocks = span_blocks(rows, cols);
  return dim3(blocks.x, blocks.y);
}

// the cloud and the mesh: a compacted stream is gathered from its organised input
int check_cloud_streams(pm_handle* h, const char* what, const float* d_normals, const float* d_normals_out,
                        const uint8_t* d_bgr8, const uint8_t* d_bgr8_out) {
  if (d_normals_out && !d_normals) {
    set_err(h, "%s: d_normals_out requested without d_normals", what);
    return PM_ERR_INVALID_ARG;
  }
  if (d_bgr8_out && !d_bgr8) {
    set_err(h, "%s: d_bgr8_out requested without d_bgr8", what);
    return PM_ERR_INVALID_ARG;
  }
  return PM_OK;
}

// Behind the checks of a stage with scratch: the handle's device, its state and its stream.
int stage_begin(pm_handle* h, const char* what, ImagingState** st, hipStream_t* stream) {
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  *st = state_of(h);
  if (!*st) {
    set_err(h, "%s: out of host memory", what);
    return PM_ERR_NOMEM;
  }
  *stream = pm_internal::stream(h);
  return PM_OK;
}

// The counts of a call, padded to 16 bytes: the words in front of a counting stage's scratch, cleared per call.
constexpr size_t kCountsHeader = 4;

// The scratch of a stage that needs the counts alone: reserved and cleared, `*d_totals` its address.
int counts_scratch(pm_handle* h, DevBuf<int>& buf, hipStream_t stream, int** d_totals) {
  PM_HIP(h, buf.reserve(sizeof(int) * kCountsHeader, stream));
  *d_totals = buf.get();
  PM_HIP(h, hipMemsetAsync(*d_totals, 0, sizeof(int) * kCountsHeader, stream));
  return PM_OK;
}

// Behind the launches of a stage that counts: the `n` (1 to 4) device totals go to the device destination and to the
// host destination where given; the host copy has landed when this returns.
int stage_counts(pm_handle* h, hipStream_t stream, const int* d_totals, int n, int* d_dst, int* dst) {
  if (d_dst) PM_HIP(h, hipMemcpyAsync(d_dst, d_totals, n * sizeof(int), hipMemcpyDeviceToDevice, stream));
  if (dst) {
    PM_HIP(h, hipMemcpyAsync(dst, d_totals, n * sizeof(int), hipMemcpyDeviceToHost, stream));
    PM_HIP(h, hipStreamSynchronize(stream));
  }
  return PM_OK;
}

}  // namespace

// ---- points, plane-mode normals and the compacted cloud behind the range stages (pm_cloud.hpp) -------------------------
int pm_backproject(pm_handle* h, const pm_cloud_camera* camera, const float* d_disp, int rows, int cols, float* d_xyz) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = check_cloud_camera(h, "pm_backproject", camera)) return rc;
  if (int rc = check_not_null(h, "pm_backproject", {{"d_disp", d_disp}, {"d_xyz", d_xyz}})) return rc;
  if (int rc = check_cloud_shape(h, "pm_backproject", rows, cols)) return rc;
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  const BackprojectArgs a = {cloud_cam(*camera), d_disp, rows, cols, d_xyz};
  const int px = kCloudBlockX * 4;
  const dim3 grid((unsigned)((cols + px - 1) / px), (unsigned)((rows + kCloudBlockY - 1) / kCloudBlockY));
  hipLaunchKernelGGL(k_backproject, grid, dim3(kCloudBlockX, kCloudBlockY), 0, pm_internal::stream(h), a);
  return launch_check(h, "backproject");
}

int pm_planes_normals(pm_handle* h, int pair, const pm_cloud_camera* camera, const float* d_disp_l, int rows, int cols,
                      float* d_normals) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (int rc = check_cloud_camera(h, "pm_planes_normals", camera)) return rc;
  if (!d_normals || pair < 0) {
    set_err(h, "pm_planes_normals: %s", !d_normals ? "null d_normals" : "negative pair");
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_cloud_shape(h, "pm_planes_normals", rows, cols)) return rc;
  return pm_internal::planes_normals(h, pair, cloud_cam(*camera), d_disp_l, rows, cols, d_normals);
}

int pm_point_cloud(pm_handle* h, const pm_cloud_camera* camera, const pm_cloud_filter* filter, const float* d_disp,
                   const float* d_normals, const uint8_t* d_bgr8, int rows, int cols, int capacity, float* d_xyz_out,
                   float* d_normals_out, uint8_t* d_bgr8_out, int32_t* d_index_out, int* d_count, int* count) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_point_cloud";
  if (int rc = check_cloud_camera(h, what, camera)) return rc;
  if (int rc = check_not_null(h, what, {{"filter", filter}, {"d_disp", d_disp}})) return rc;
  if (int rc = check_cloud_filter(h, what, filter)) return rc;
  if (capacity < 0) {
    set_err(h, "%s: capacity %d must be >= 0", what, capacity);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_cloud_streams(h, what, d_normals, d_normals_out, d_bgr8, d_bgr8_out)) return rc;
  if (int rc = check_cloud_shape(h, what, rows, cols)) return rc;
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  const CloudArgs a = cloud_args(*camera, *filter, d_disp, rows, cols);
  const int blocks = (int)((a.items + kCloudBlock - 1) / kCloudBlock);
  PM_HIP(h, st->cloud_blocks.reserve(sizeof(int) * ((size_t)blocks + 1), stream));
  int* d_total = st->cloud_blocks.get();
  int* d_blocks = d_total + 1;
  const CloudStreams s = {d_normals, d_bgr8, d_xyz_out, d_normals_out, d_bgr8_out, d_index_out, capacity};
  hipLaunchKernelGGL(k_cloud_count, dim3((unsigned)blocks), dim3(kCloudBlock), 0, stream, a, d_blocks);
  hipLaunchKernelGGL(k_cloud_offsets, dim3(1), dim3(kCloudScanThreads), 0, stream, d_blocks, blocks, d_total, d_count);
  if (capacity > 0 && (d_xyz_out || d_normals_out || d_bgr8_out || d_index_out))
    hipLaunchKernelGGL(k_cloud_scatter, dim3((unsigned)blocks), dim3(kCloudBlock), 0, stream, a, (const int*)d_blocks, s);
  if (int rc = launch_check(h, "point cloud")) return rc;
  return stage_counts(h, stream, d_total, 1, nullptr, count);  // k_cloud_offsets wrote d_count
}

void pm_debug_cloud_constants(int* items_per_block, int* blocks_per_scan_pass) {
  if (items_per_block) *items_per_block = kCloudBlock;
  if (blocks_per_scan_pass) *blocks_per_scan_pass = kCloudScanThreads;
}

// ---- normals for scalar-mode maps: the windowed plane fit (pm_normals_fit.hpp) ---------------------------------------------
namespace {

template <int R>
void launch_normals_fit(const NormalsFitArgs& a, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL(k_normals_fit<R>, grid, dim3(kNormalsFitTileCols, kNormalsFitTileRows), 0, stream, a);
}

}  // namespace

int pm_disparity_normals(pm_handle* h, const pm_cloud_camera* camera, const pm_normals_fit* fit, const float* d_disp, int rows,
                         int cols, float* d_normals, float* d_planes, uint8_t* d_support) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_disparity_normals";
  if (int rc = check_not_null(h, what, {{"fit", fit}, {"d_disp", d_disp}})) return rc;
  if (int rc = check_any_output(h, what, {d_normals, d_planes, d_support}, "d_normals, d_planes and d_support", true)) return rc;
  if (d_normals)  // the camera is read for the normals alone
    if (int rc = check_cloud_camera(h, what, camera)) return rc;
  if (fit->radius < 1 || fit->radius > kNormalsFitMaxRadius) {
    set_err(h, "%s: radius %d outside 1..%d", what, fit->radius, kNormalsFitMaxRadius);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_max_diff(h, what, fit->max_diff)) return rc;
  const int window = (2 * fit->radius + 1) * (2 * fit->radius + 1);
  if (fit->min_support < 3 || fit->min_support > window) {
    set_err(h, "%s: min_support %d outside 3..%d", what, fit->min_support, window);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_cloud_shape(h, what, rows, cols)) return rc;
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  const NormalsFitArgs a = {d_normals ? cloud_cam(*camera) : CloudCam{1.0, 1.0, 0.0, 0.0, 1.0}, d_disp, rows, cols, fit->radius,
                            fit->max_diff, fit->min_support, d_normals, d_planes, d_support};
  const dim3 grid((unsigned)((cols + kNormalsFitTileCols - 1) / kNormalsFitTileCols),
                  (unsigned)((rows + kNormalsFitTileRows - 1) / kNormalsFitTileRows));
  hipStream_t stream = pm_internal::stream(h);
#ifdef PM_TUNING
  static const bool runtime_radius = pm::tune_env("PM_NORMALS_FIT_RUNTIME_RADIUS") != nullptr;
  if (runtime_radius) {
    hipLaunchKernelGGL(k_normals_fit_any, grid, dim3(kNormalsFitTileCols, kNormalsFitTileRows), 0, stream, a);
    return launch_check(h, "normals fit");
  }
#endif
  switch (fit->radius) {
    case 1: launch_normals_fit<1>(a, grid, stream); break;
    case 2: launch_normals_fit<2>(a, grid, stream); break;
    case 3: launch_normals_fit<3>(a, grid, stream); break;
    case 4: launch_normals_fit<4>(a, grid, stream); break;
    case 5: launch_normals_fit<5>(a, grid, stream); break;
    case 6: launch_normals_fit<6>(a, grid, stream); break;
    default: launch_normals_fit<7>(a, grid, stream); break;
  }
  return launch_check(h, "normals fit");
}

void pm_debug_normals_fit_constants(int* tile_cols, int* tile_rows, int* pixels_per_thread) {
  if (tile_cols) *tile_cols = kNormalsFitTileCols;
  if (tile_rows) *tile_rows = kNormalsFitTileRows;
  if (pixels_per_thread) *pixels_per_thread = 1;
}

// ---- speckle filter: connected components of similar disparity (pm_speckle.hpp) ------------------------------------------
int pm_filter_speckles(pm_handle* h, const pm_speckle_filter* filter, const float* d_disp, int rows, int cols, float* d_out,
                       int32_t* d_labels, int32_t* d_sizes, int* d_removed, int* removed) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_filter_speckles";
  if (int rc = check_not_null(h, what, {{"filter", filter}, {"d_disp", d_disp}})) return rc;
  if (int rc = check_any_output(h, what, {d_out, d_labels, d_sizes, d_removed, removed},
                                "d_out, d_labels, d_sizes, d_removed and removed", true))
    return rc;
  if (int rc = check_max_diff(h, what, filter->max_diff)) return rc;
  if (filter->max_size < 0) {
    set_err(h, "%s: max_size %d must be >= 0", what, filter->max_size);
    return PM_ERR_INVALID_ARG;
  }
  // its own shape check: the grids are one-dimensional, so only the pixel index bounds the map
  if (rows < 1 || cols < 1) {
    set_err(h, "%s: empty image (%dx%d)", what, cols, rows);
    return PM_ERR_INVALID_ARG;
  }
  if ((long long)rows * cols > INT32_MAX) {
    set_err(h, "%s: %dx%d pixels exceed a 32-bit pixel index", what, cols, rows);
    return PM_ERR_SIZE;
  }
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  const int pixels = rows * cols;
  PM_HIP(h, st->speckle_buf.reserve(sizeof(int) * (kCountsHeader + 2 * (size_t)pixels), stream));
  int* d_total = st->speckle_buf.get();
  const SpeckleArgs a = {d_disp, rows, cols, filter->max_diff, d_total + kCountsHeader, d_total + kCountsHeader + pixels};
  const SpeckleOut o = {d_out, d_labels, d_sizes, filter->max_size};
  const int tiles_x = speckle_tiles_x(cols);
  const long long tiles = (long long)tiles_x * speckle_tiles_y(rows), items = speckle_merge_items(rows, cols);
  const unsigned per_pixel = (unsigned)(((long long)pixels + kSpeckleBlock - 1) / kSpeckleBlock);
  PM_HIP(h, hipMemsetAsync(d_total, 0, sizeof(int) * kCountsHeader, stream));
  hipLaunchKernelGGL(k_speckle_local, dim3((unsigned)tiles), dim3(kSpeckleTileCols, kSpeckleTileRows), 0, stream, a, tiles_x);
  if (items > 0)
    hipLaunchKernelGGL(k_speckle_merge, dim3((unsigned)((items + kSpeckleBlock - 1) / kSpeckleBlock)), dim3(kSpeckleBlock), 0,
                       stream, a, items);
  hipLaunchKernelGGL(k_speckle_flatten, dim3(per_pixel), dim3(kSpeckleBlock), 0, stream, a, pixels);
  hipLaunchKernelGGL(k_speckle_apply, dim3(per_pixel), dim3(kSpeckleBlock), 0, stream, a, o, pixels, d_total);
  if (int rc = launch_check(h, "speckle filter")) return rc;
  return stage_counts(h, stream, d_total, 1, d_removed, removed);
}

void pm_debug_speckle_constants(int* tile_cols, int* tile_rows) {
  if (tile_cols) *tile_cols = kSpeckleTileCols;
  if (tile_rows) *tile_rows = kSpeckleTileRows;
}

// ---- grid mesh: vertices and triangles of a disparity map's stride grid (pm_mesh.hpp) -------------------------------------
int pm_grid_mesh(pm_handle* h, const pm_cloud_camera* camera, const pm_cloud_filter* filter, const pm_mesh_options* options,
                 const float* d_disp, const float* d_normals, const uint8_t* d_bgr8, int rows, int cols, int vertex_capacity,
                 int tri_capacity, float* d_xyz_out, float* d_normals_out, uint8_t* d_bgr8_out, int32_t* d_index_out,
                 int32_t* d_tri_out, int* d_counts, int* counts) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_grid_mesh";
  if (int rc = check_cloud_camera(h, what, camera)) return rc;
  if (int rc = check_not_null(h, what, {{"filter", filter}, {"options", options}, {"d_disp", d_disp}})) return rc;
  if (int rc = check_cloud_filter(h, what, filter)) return rc;
  if (int rc = check_max_diff(h, what, options->max_diff)) return rc;
  if (options->vertices != PM_MESH_VERTICES_ALL && options->vertices != PM_MESH_VERTICES_REFERENCED) {
    set_err(h, "%s: vertices %d is neither PM_MESH_VERTICES_ALL nor PM_MESH_VERTICES_REFERENCED", what, options->vertices);
    return PM_ERR_INVALID_ARG;
  }
  if (vertex_capacity < 0 || tri_capacity < 0) {
    set_err(h, "%s: %s %d must be >= 0", what, vertex_capacity < 0 ? "vertex_capacity" : "tri_capacity",
            vertex_capacity < 0 ? vertex_capacity : tri_capacity);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_cloud_streams(h, what, d_normals, d_normals_out, d_bgr8, d_bgr8_out)) return rc;
  if (int rc = check_cloud_shape(h, what, rows, cols)) return rc;
  const int sub_rows = cloud_grid(rows, filter->stride);
  const MeshArgs a = {cloud_args(*camera, *filter, d_disp, rows, cols), sub_rows, options->max_diff,
                      options->vertices == PM_MESH_VERTICES_REFERENCED};
  const int sub_cols = a.c.sub_cols;
  if (2 * ((long long)(sub_rows - 1) * (sub_cols - 1)) > INT32_MAX) {
    set_err(h, "%s: the %dx%d grid has more than 2^31 - 1 possible triangles", what, sub_cols, sub_rows);
    return PM_ERR_SIZE;
  }
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  const int blocks = sub_rows * mesh_segments(sub_cols);  // <= rows * ceil(cols / 256): far below 2^31 (check_cloud_shape)
  PM_HIP(h, st->mesh_buf.reserve(sizeof(int) * (2 + 2 * (size_t)blocks + (size_t)a.c.items), stream));
  int* d_totals = st->mesh_buf.get();
  int* d_vertex_blocks = d_totals + 2;
  int* d_tri_blocks = d_vertex_blocks + blocks;
  int32_t* d_slot_map = d_tri_blocks + blocks;
  const bool want_vertices = vertex_capacity > 0 && (d_xyz_out || d_normals_out || d_bgr8_out || d_index_out);
  const bool want_tris = tri_capacity > 0 && d_tri_out;
  const CloudStreams s = {d_normals, d_bgr8, d_xyz_out, d_normals_out, d_bgr8_out, d_index_out, want_vertices ? vertex_capacity : 0};
  const dim3 grid((unsigned)blocks), block(kMeshBlock);
  hipLaunchKernelGGL(k_mesh_count, grid, block, 0, stream, a, d_vertex_blocks, d_tri_blocks);
  hipLaunchKernelGGL(k_cloud_offsets, dim3(1), dim3(kCloudScanThreads), 0, stream, d_vertex_blocks, blocks, d_totals,
                     d_counts);
  hipLaunchKernelGGL(k_cloud_offsets, dim3(1), dim3(kCloudScanThreads), 0, stream, d_tri_blocks, blocks, d_totals + 1,
                     d_counts ? d_counts + 1 : nullptr);
  if (want_vertices || want_tris)  // the triangles name the slots this launch leaves in the slot map
    hipLaunchKernelGGL(k_mesh_vertices, grid, block, 0, stream, a, (const int*)d_vertex_blocks, s, d_slot_map);
  if (want_tris)
    hipLaunchKernelGGL(k_mesh_triangles, grid, block, 0, stream, a, (const int*)d_tri_blocks, (const int32_t*)d_slot_map,
                       d_tri_out, tri_capacity);
  if (int rc = launch_check(h, "grid mesh")) return rc;
  return stage_counts(h, stream, d_totals, 2, nullptr, counts);  // k_cloud_offsets wrote d_counts
}

void pm_debug_mesh_constants(int* items_per_block, int* blocks_per_scan_pass) {
  if (items_per_block) *items_per_block = kMeshBlock;
  if (blocks_per_scan_pass) *blocks_per_scan_pass = kCloudScanThreads;
}

// ---- temporal seeds: a map carried into the next frame's two seed maps (pm_reproject.hpp) ------------------------------------
int pm_reproject_disparity(pm_handle* h, const pm_cloud_camera* camera, const pm_motion* motion,
                           const pm_reproject_options* options, const float* d_disp, int rows, int cols, float* d_seed_l,
                           float* d_seed_r, int* d_counts, int* counts) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_reproject_disparity";
  if (int rc = check_cloud_camera(h, what, camera)) return rc;
  if (int rc = check_not_null(h, what, {{"motion", motion}, {"options", options}, {"d_disp", d_disp}})) return rc;
  if (int rc = check_motion(h, what, *motion, "the motion")) return rc;
  if (int rc = check_disp_limits(h, what, options->min_disp, options->max_disp)) return rc;
  if (options->close_radius < 0 || options->close_radius > kReprojectMaxRadius) {
    set_err(h, "%s: close_radius %d must be 0 .. %d", what, options->close_radius, kReprojectMaxRadius);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_cloud_shape(h, what, rows, cols)) return rc;
  if (int rc = check_any_output(h, what, {d_seed_l, d_seed_r, d_counts, counts}, "d_seed_l, d_seed_r, d_counts and counts"))
    return rc;
  if (d_seed_l == d_disp || d_seed_r == d_disp) {
    set_err(h, "%s: %s must not alias d_disp", what, d_seed_l == d_disp ? "d_seed_l" : "d_seed_r");
    return PM_ERR_INVALID_ARG;
  }
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  const size_t px = (size_t)rows * cols;
  const size_t cleared = kCountsHeader + 2 * px;
  PM_HIP(h, st->reproject_buf.reserve(sizeof(unsigned) * (cleared + (d_seed_l ? 0 : px)), stream));
  unsigned* base = st->reproject_buf.get();
  int* d_totals = reinterpret_cast<int*>(base);
  unsigned* splat_l = base + kCountsHeader;
  unsigned* splat_r = splat_l + px;
  unsigned* closed_l = d_seed_l ? reinterpret_cast<unsigned*>(d_seed_l) : splat_r + px;
  PM_HIP(h, hipMemsetAsync(base, 0, sizeof(unsigned) * cleared, stream));
  ReprojectArgs a = {cloud_cam(*camera), {}, {}, options->min_disp, options->max_disp, d_disp, rows, cols, splat_l};
  set_motion(a.R, a.t, motion);
  const dim3 block(kReprojectBlockX, kReprojectBlockY);
  const dim3 splat_grid = span_grid(rows, cols);
  const dim3 tile_grid((unsigned)((cols + kReprojectTileW - 1) / kReprojectTileW),
                       (unsigned)((rows + kReprojectTileH - 1) / kReprojectTileH));
  const int r = options->close_radius;
  hipLaunchKernelGGL(k_reproject_splat, splat_grid, block, 0, stream, a);
  hipLaunchKernelGGL(k_reproject_finish, tile_grid, block, 0, stream,
                     ReprojectFinishArgs{splat_l, closed_l, rows, cols, r, d_totals});
  if (d_seed_r || d_counts || counts) {  // the right view: from the CLOSED left seed
    hipLaunchKernelGGL(k_reproject_splat_right, splat_grid, block, 0, stream,
                       ReprojectRightArgs{reinterpret_cast<const float*>(closed_l), rows, cols, splat_r});
    hipLaunchKernelGGL(k_reproject_finish, tile_grid, block, 0, stream,
                       ReprojectFinishArgs{splat_r, reinterpret_cast<unsigned*>(d_seed_r), rows, cols, r, d_totals + 1});
  }
  if (int rc = launch_check(h, "reproject disparity")) return rc;
  return stage_counts(h, stream, d_totals, 2, d_counts, counts);
}

void pm_debug_reproject_constants(int* tile_w, int* tile_h) {
  if (tile_w) *tile_w = kReprojectTileW;
  if (tile_h) *tile_h = kReprojectTileH;
}

// ---- geometric consistency: a map judged by earlier maps of its sequence (pm_consistency.hpp) -------------------------------
namespace {
template <int RADIUS>
void launch_consistency(const ConsistencyArgs& a, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL(k_consistency<RADIUS>, grid, dim3(kConsistencyBlockX, kConsistencyBlockY), 0, stream, a);
}
}  // namespace

int pm_filter_consistency(pm_handle* h, const pm_cloud_camera* camera, const pm_consistency_options* options,
                          const float* d_disp, int n_sources, const float* const* d_sources, const pm_motion* motions, int rows,
                          int cols, float* d_out, uint16_t* d_classes, float* d_residual, int* d_counts, int* counts) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_filter_consistency";
  if (int rc = check_cloud_camera(h, what, camera)) return rc;
  if (int rc = check_not_null(h, what, {{"options", options}, {"d_disp", d_disp}, {"d_sources", d_sources}, {"motions", motions}}))
    return rc;
  if (int rc = check_sources(h, what, n_sources, d_sources, motions)) return rc;
  if (int rc = check_votes(h, what, options->max_diff, options->radius, options->min_consistent, options->max_conflicts, n_sources))
    return rc;
  if (int rc = check_cloud_shape(h, what, rows, cols)) return rc;
  if (int rc = check_any_output(h, what, {d_out, d_classes, d_residual, d_counts, counts},
                                "d_out, d_classes, d_residual, d_counts and counts"))
    return rc;
  for (int k = 0; d_out && k < n_sources; ++k)
    if (d_out == d_sources[k]) {  // a pixel of a source is read by other pixels' lookups
      set_err(h, "%s: d_out must not alias d_sources[%d]", what, k);
      return PM_ERR_INVALID_ARG;
    }
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  int* d_totals = nullptr;
  if (int rc = counts_scratch(h, st->consistency_counts, stream, &d_totals)) return rc;
  ConsistencyArgs a = {};
  a.cam = cloud_cam(*camera);
  a.disp = d_disp, a.rows = rows, a.cols = cols, a.n = n_sources;
  a.max_diff = options->max_diff, a.min_consistent = options->min_consistent, a.max_conflicts = options->max_conflicts;
  a.out = d_out, a.classes = d_classes, a.residual = d_residual, a.counts = d_totals;
  for (int k = 0; k < n_sources; ++k) {
    set_motion(a.src[k].R, a.src[k].t, &motions[k]);
    a.src[k].map = d_sources[k];
  }
  const dim3 grid = span_grid(rows, cols);
  switch (options->radius) {
    case 0: launch_consistency<0>(a, grid, stream); break;
    case 1: launch_consistency<1>(a, grid, stream); break;
    default: launch_consistency<2>(a, grid, stream); break;
  }
  if (int rc = launch_check(h, "consistency filter")) return rc;
  return stage_counts(h, stream, d_totals, 2, d_counts, counts);
}

// ---- matching confidence: the functor evaluated again around a map's answer (pm_confidence.hpp) -----------------------------
namespace {
template <int PW, int PH>
void launch_confidence(const ConfidenceArgs& a, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((k_confidence<PW, PH>), grid, dim3(kConfThreads), 0, stream, a);
}
}  // namespace

int pm_disparity_confidence(pm_handle* h, const pm_confidence_options* options, const uint8_t* d_left, const uint8_t* d_right,
                            const float* d_disp_l, const float* d_disp_r, int rows, int cols, float* d_out, float* d_measures,
                            uint8_t* d_flags, int* d_counts, int* counts) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_disparity_confidence";
  if (int rc = check_not_null(h, what, {{"options", options}, {"d_left", d_left}, {"d_right", d_right}, {"d_disp_l", d_disp_l}}))
    return rc;
  if (int rc = check_any_output(h, what, {d_out, d_measures, d_flags, d_counts, counts},
                                "d_out, d_measures, d_flags, d_counts and counts"))
    return rc;
  const int pw = options->patch_w, ph = options->patch_h;
  if (pw < 3 || pw > PM_MAX_PATCH || pw % 2 == 0 || ph < 3 || ph > PM_MAX_PATCH || ph % 2 == 0) {
    const bool w_bad = pw < 3 || pw > PM_MAX_PATCH || pw % 2 == 0;
    set_err(h, "%s: %s %d must be odd and within 3..%d", what, w_bad ? "patch_w" : "patch_h", w_bad ? pw : ph, PM_MAX_PATCH);
    return PM_ERR_INVALID_ARG;
  }
  if (std::isnan(options->max_cost) || std::isnan(options->min_margin) || std::isnan(options->min_bg_margin) ||
      std::isnan(options->max_lr_diff)) {
    set_err(h, "%s: %s must not be NaN", what,
            std::isnan(options->max_cost) ? "max_cost" : std::isnan(options->min_margin) ? "min_margin"
            : std::isnan(options->min_bg_margin) ? "min_bg_margin" : "max_lr_diff");
    return PM_ERR_INVALID_ARG;
  }
  if (options->drop_unmeasured != 0 && options->drop_unmeasured != 1) {
    set_err(h, "%s: drop_unmeasured %d must be 0 or 1", what, options->drop_unmeasured);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_cloud_shape(h, what, rows, cols)) return rc;
  if (d_out && d_out == d_disp_r) {  // a pixel of the right map is read by other pixels' lookups
    set_err(h, "%s: d_out must not alias d_disp_r", what);
    return PM_ERR_INVALID_ARG;
  }
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  const size_t px = (size_t)rows * cols;
  PM_HIP(h, st->confidence_buf.reserve(sizeof(int) * (kCountsHeader + px + (px + 3) / 4), stream));
  int* d_totals = st->confidence_buf.get();
  float* d_gr = reinterpret_cast<float*>(d_totals + kCountsHeader);
  uint8_t* d_gl8 = reinterpret_cast<uint8_t*>(d_gr + px);
  const pm_params& p = pm_internal::params(h);
  ConfidenceArgs a = {};
  a.left = d_left, a.right = d_right, a.gl8 = d_gl8, a.gr = d_gr, a.disp_l = d_disp_l, a.disp_r = d_disp_r;
  a.rows = rows, a.cols = cols, a.pw = pw, a.ph = ph;
  a.max_cost = options->max_cost, a.min_margin = options->min_margin, a.min_bg_margin = options->min_bg_margin;
  a.max_lr_diff = options->max_lr_diff, a.drop_unmeasured = options->drop_unmeasured;
  a.cp = confidence_cost_params(p.functor_alpha, p.functor_tau_color, p.functor_tau_grad, pw, ph);
  a.out = d_out, a.measures = d_measures, a.flags = d_flags, a.counts = d_totals;
  PM_HIP(h, hipMemsetAsync(d_totals, 0, sizeof(int) * kCountsHeader, stream));
  static_assert(kConfGradBlockY == kCloudBlockY && kConfTileH >= kCloudBlockY, "check_cloud_shape bounds both grids");
  hipLaunchKernelGGL(k_confidence_grad,
                     dim3((unsigned)((cols + kConfGradBlockX - 1) / kConfGradBlockX), (unsigned)((rows + kConfGradBlockY - 1) / kConfGradBlockY)),
                     dim3(kConfGradBlockX, kConfGradBlockY), 0, stream, d_left, d_right, rows, cols, d_gl8, d_gr);
  const dim3 grid((unsigned)((cols + kConfTileW - 1) / kConfTileW), (unsigned)((rows + kConfTileH - 1) / kConfTileH));
  switch (pw == ph ? pw : 0) {
    case 3: launch_confidence<3, 3>(a, grid, stream); break;
    case 5: launch_confidence<5, 5>(a, grid, stream); break;
    case 7: launch_confidence<7, 7>(a, grid, stream); break;
    case 9: launch_confidence<9, 9>(a, grid, stream); break;
    case 11: launch_confidence<11, 11>(a, grid, stream); break;
    default: launch_confidence<0, 0>(a, grid, stream); break;
  }
  if (int rc = launch_check(h, "disparity confidence")) return rc;
  return stage_counts(h, stream, d_totals, 3, d_counts, counts);
}

void pm_debug_confidence_constants(int* tile_w, int* tile_h, int* target_cols) {
  if (tile_w) *tile_w = kConfTileW;
  if (tile_h) *tile_h = kConfTileH;
  if (target_cols) *target_cols = kConfTileRW;
}

// ---- sequence fusion: a map refined by, and filled from, earlier maps of its sequence (pm_fuse.hpp) ---------------------------
namespace {
template <int RADIUS>
void launch_fuse(const FuseArgs& a, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL(k_fuse<RADIUS>, grid, dim3(kFuseBlockX, kFuseBlockY), 0, stream, a);
}
}  // namespace

int pm_fuse_disparity(pm_handle* h, const pm_cloud_camera* camera, const pm_fuse_options* options, const float* d_disp,
                      const float* d_weight, int n_sources, const float* const* d_sources, const pm_motion* motions,
                      const float* const* d_source_weights, int rows, int cols, float* d_out, uint8_t* d_count,
                      float* d_spread, uint8_t* d_flags, int* d_counts, int* counts) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_fuse_disparity";
  if (int rc = check_cloud_camera(h, what, camera)) return rc;
  if (int rc = check_not_null(h, what, {{"options", options}, {"d_disp", d_disp}, {"d_sources", d_sources}, {"motions", motions}}))
    return rc;
  if (int rc = check_sources(h, what, n_sources, d_sources, motions)) return rc;
  if (int rc = check_votes(h, what, options->max_diff, options->radius, options->min_consistent, options->max_conflicts, n_sources))
    return rc;
  if (options->fill_min_sources < 0 || options->fill_min_sources > n_sources) {
    set_err(h, "%s: fill_min_sources %d outside 0..n_sources (%d)", what, options->fill_min_sources, n_sources);
    return PM_ERR_INVALID_ARG;
  }
  if (!std::isfinite(options->fill_max_diff) || options->fill_max_diff < 0.f) {
    set_err(h, "%s: fill_max_diff must be finite and >= 0", what);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_cloud_shape(h, what, rows, cols)) return rc;
  if (int rc = check_any_output(h, what, {d_out, d_count, d_spread, d_flags, d_counts, counts},
                                "d_out, d_count, d_spread, d_flags, d_counts and counts"))
    return rc;
  const void* const outs[4] = {d_out, d_count, d_spread, d_flags};
  static const char* const out_names[4] = {"d_out", "d_count", "d_spread", "d_flags"};
  for (int o = 0; o < 4; ++o)
    for (int k = 0; outs[o] && k < n_sources; ++k) {  // a pixel of a source is read by other pixels' lookups
      const bool map = outs[o] == d_sources[k];
      if (map || (d_source_weights && outs[o] == d_source_weights[k])) {
        set_err(h, "%s: %s must not alias %s[%d]", what, out_names[o], map ? "d_sources" : "d_source_weights", k);
        return PM_ERR_INVALID_ARG;
      }
    }
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  const bool fill = options->fill_min_sources >= 1;
  const size_t px = (size_t)rows * cols;
  const size_t words = kCountsHeader + (fill ? (size_t)n_sources * px : 0);
  PM_HIP(h, st->fuse_buf.reserve(sizeof(unsigned) * words, stream));
  unsigned* base = st->fuse_buf.get();
  unsigned* d_splat = base + kCountsHeader;
  FuseArgs a = {};
  a.cam = cloud_cam(*camera);
  a.disp = d_disp, a.weight = d_weight, a.rows = rows, a.cols = cols, a.n = n_sources;
  a.max_diff = options->max_diff, a.min_consistent = options->min_consistent, a.max_conflicts = options->max_conflicts;
  a.fill_min_sources = options->fill_min_sources, a.fill_max_diff = options->fill_max_diff;
  a.splat = d_splat, a.px = px;
  a.out = d_out, a.count = d_count, a.spread = d_spread, a.flags = d_flags, a.counts = reinterpret_cast<int*>(base);
  FuseSplatArgs sa = {};
  sa.cam = a.cam, sa.rows = rows, sa.cols = cols, sa.splat = d_splat, sa.px = px;
  for (int k = 0; k < n_sources; ++k) {
    set_motion(a.src[k].R, a.src[k].t, &motions[k]);
    a.src[k].map = d_sources[k];
    a.src[k].weight = d_source_weights ? d_source_weights[k] : nullptr;
    motion_inverse(motions[k].R, motions[k].t, sa.src[k].R, sa.src[k].t);  // in binary64 (not contracted: -ffp-contract=off)
    sa.src[k].map = d_sources[k];
  }
  PM_HIP(h, hipMemsetAsync(base, 0, sizeof(unsigned) * words, stream));
  const dim3 block(kFuseBlockX, kFuseBlockY);
  const dim3 grid = span_grid(rows, cols);
  if (fill) hipLaunchKernelGGL(k_fuse_splat, dim3(grid.x, grid.y, (unsigned)n_sources), block, 0, stream, sa);
  switch (options->radius) {
    case 0: launch_fuse<0>(a, grid, stream); break;
    case 1: launch_fuse<1>(a, grid, stream); break;
    default: launch_fuse<2>(a, grid, stream); break;
  }
  if (int rc = launch_check(h, "fuse disparity")) return rc;
  return stage_counts(h, stream, reinterpret_cast<const int*>(base), 4, d_counts, counts);
}

// ---- a persistent world-frame model: a TSDF volume integrated from maps and raycast back (pm_tsdf.hpp) ------------------------
namespace {
// the volume's voxels, or 0 where a dimension is < 1 or they exceed 2^31 - 1
size_t tsdf_voxels(const pm_tsdf_volume& v) {
  if (v.nx < 1 || v.ny < 1 || v.nz < 1) return 0;
  const size_t xy = (size_t)v.nx * (size_t)v.ny;
  if (xy > (size_t)INT32_MAX || xy * (size_t)v.nz > (size_t)INT32_MAX) return 0;
  return xy * (size_t)v.nz;
}

const char* tsdf_volume_fault(const pm_tsdf_volume& v) {
  if (v.nx < 1 || v.ny < 1 || v.nz < 1) return "nx, ny and nz of the volume must be >= 1";
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(v.origin[i])) return "origin of the volume is not finite";
  if (!std::isfinite(v.voxel) || !(v.voxel > 0.0)) return "voxel of the volume must be finite and > 0";
  if (!std::isfinite(v.trunc) || !(v.trunc > 0.0)) return "trunc of the volume must be finite and > 0";
  if (!std::isfinite(v.max_weight) || !(v.max_weight > 0.f)) return "max_weight of the volume must be finite and > 0";
  return nullptr;
}

// what pm_tsdf_integrate and pm_tsdf_raycast check in the same order: camera, the null pointers, the volume, the pose
int check_tsdf_common(pm_handle* h, const char* what, const pm_cloud_camera* camera, const pm_tsdf_volume* volume,
                      const pm_motion* pose, const void* options, const void* d_voxels, const char* voxels_name = "d_voxels") {
  if (int rc = check_cloud_camera(h, what, camera)) return rc;
  if (int rc = check_not_null(h, what, {{"volume", volume}, {"pose", pose}, {"options", options}, {voxels_name, d_voxels}}))
    return rc;
  if (const char* fault = tsdf_volume_fault(*volume)) {
    set_err(h, "%s: %s", what, fault);
    return PM_ERR_INVALID_ARG;
  }
  return check_motion(h, what, *pose, "the pose");
}

int check_tsdf_size(pm_handle* h, const char* what, const pm_tsdf_volume& v) {
  if (tsdf_voxels(v) == 0) {
    set_err(h, "%s: %dx%dx%d voxels exceed 2^31 - 1", what, v.nx, v.ny, v.nz);
    return PM_ERR_SIZE;
  }
  return PM_OK;
}

// what pm_tsdf_integrate and pm_tsdf_integrate_color check in the same order; Options begins with min_disp and max_range
template <typename Options>
int check_tsdf_integrate(pm_handle* h, const char* what, const pm_cloud_camera* camera, const pm_tsdf_volume* volume,
                         const pm_motion* pose, const Options* options, const float* d_disp, int rows, int cols,
                         const void* d_voxels) {
  if (int rc = check_tsdf_common(h, what, camera, volume, pose, options, d_voxels)) return rc;
  if (int rc = check_not_null(h, what, {{"d_disp", d_disp}})) return rc;
  if (std::isnan(options->min_disp) || options->min_disp < 0.f) {
    set_err(h, "%s: min_disp must not be NaN or negative", what);
    return PM_ERR_INVALID_ARG;
  }
  if (!(options->max_range >= 0.f)) {
    set_err(h, "%s: max_range must be >= 0 (0 = no limit)", what);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_cloud_shape(h, what, rows, cols)) return rc;
  return check_tsdf_size(h, what, *volume);
}

// the block count of k_tsdf_integrate and k_tsdf_integrate_color
dim3 tsdf_span_grid(const pm_tsdf_volume& v) {
  const size_t spans = (((size_t)v.nx + kTsdfLanes - 1) / kTsdfLanes) * (size_t)v.ny * (size_t)v.nz;
  const size_t blocks = (spans + kTsdfBlockY - 1) / kTsdfBlockY;
  return dim3((unsigned)(blocks < kTsdfMaxBlocks ? blocks : kTsdfMaxBlocks));
}
}  // namespace

size_t pm_tsdf_bytes(const pm_tsdf_volume* volume) {
  if (!volume || tsdf_volume_fault(*volume)) return 0;
  return tsdf_voxels(*volume) * sizeof(TsdfVoxel);
}

int pm_tsdf_clear(pm_handle* h, const pm_tsdf_volume* volume, void* d_voxels) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_tsdf_clear";
  if (int rc = check_not_null(h, what, {{"volume", volume}, {"d_voxels", d_voxels}})) return rc;
  if (const char* fault = tsdf_volume_fault(*volume)) {
    set_err(h, "%s: %s", what, fault);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_tsdf_size(h, what, *volume)) return rc;
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  PM_HIP(h, hipMemsetAsync(d_voxels, 0, tsdf_voxels(*volume) * sizeof(TsdfVoxel), pm_internal::stream(h)));  // {+0.0f, +0.0f}
  return PM_OK;
}

int pm_tsdf_integrate(pm_handle* h, const pm_cloud_camera* camera, const pm_tsdf_volume* volume, const pm_motion* pose,
                      const pm_tsdf_integrate_options* options, const float* d_disp, const float* d_weight, int rows, int cols,
                      void* d_voxels, int* d_counts, int* counts) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_tsdf_integrate";
  if (int rc = check_tsdf_integrate(h, what, camera, volume, pose, options, d_disp, rows, cols, d_voxels)) return rc;
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  int* d_totals = nullptr;
  if (int rc = counts_scratch(h, st->tsdf_counts, stream, &d_totals)) return rc;
  TsdfIntegrateArgs a = {};
  a.cam = cloud_cam(*camera);
  a.grid = tsdf_grid(*volume);
  set_motion(a.R, a.t, pose);
  a.min_disp = options->min_disp, a.max_range = options->max_range;
  a.disp = d_disp, a.weight = d_weight, a.rows = rows, a.cols = cols;
  a.voxels = static_cast<TsdfVoxel*>(d_voxels), a.counts = d_totals;
  hipLaunchKernelGGL(k_tsdf_integrate, tsdf_span_grid(*volume), dim3(kTsdfBlockX, kTsdfBlockY), 0, stream, a);
  if (int rc = launch_check(h, "tsdf integrate")) return rc;
  return stage_counts(h, stream, d_totals, 2, d_counts, counts);
}

int pm_tsdf_raycast(pm_handle* h, const pm_cloud_camera* camera, const pm_tsdf_volume* volume, const pm_motion* pose,
                    const pm_tsdf_raycast_options* options, const void* d_voxels, int rows, int cols, float* d_disp_out,
                    float* d_normals_out, int* d_counts, int* counts) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_tsdf_raycast";
  if (int rc = check_tsdf_common(h, what, camera, volume, pose, options, d_voxels)) return rc;
  if (!(options->step > 0.f && options->step <= 1.f)) {
    set_err(h, "%s: step must lie in (0, 1]", what);
    return PM_ERR_INVALID_ARG;
  }
  if (!std::isfinite(options->min_range) || !std::isfinite(options->max_range) || !(options->min_range > 0.f) ||
      !(options->min_range < options->max_range)) {
    set_err(h, "%s: min_range and max_range must be finite with 0 < min_range < max_range", what);
    return PM_ERR_INVALID_ARG;
  }
  if (std::isnan(options->min_weight) || options->min_weight < 0.f) {
    set_err(h, "%s: min_weight must not be NaN or negative", what);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_cloud_shape(h, what, rows, cols)) return rc;
  if (int rc = check_any_output(h, what, {d_disp_out, d_normals_out, d_counts, counts},
                                "d_disp_out, d_normals_out, d_counts and counts"))
    return rc;
  if (int rc = check_tsdf_size(h, what, *volume)) return rc;
  TsdfRaycastArgs a = {};
  a.cam = cloud_cam(*camera);
  a.grid = tsdf_grid(*volume);
  set_motion(a.R, nullptr, pose);
  motion_inverse(pose->R, pose->t, a.Ri, a.c);  // in binary64 (not contracted: -ffp-contract=off)
  a.min_range = (double)options->min_range, a.max_range = (double)options->max_range;
  a.ds = (double)options->step * volume->trunc;
  a.min_weight = options->min_weight;
  a.n_samples = tsdf_sample_count(a.min_range, a.max_range, a.ds);
  if (a.n_samples < 0) {
    set_err(h, "%s: step * trunc puts more than 65536 samples between min_range and max_range", what);
    return PM_ERR_SIZE;
  }
  a.voxels = static_cast<const TsdfVoxel*>(d_voxels), a.rows = rows, a.cols = cols;
  a.disp_out = d_disp_out, a.normals_out = d_normals_out;
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  int* d_totals = nullptr;
  if (int rc = counts_scratch(h, st->tsdf_counts, stream, &d_totals)) return rc;
  a.counts = d_totals;
  const dim3 grid((unsigned)((cols + kTsdfLanes - 1) / kTsdfLanes), (unsigned)((rows + kTsdfBlockY - 1) / kTsdfBlockY));
  hipLaunchKernelGGL(k_tsdf_raycast, grid, dim3(kTsdfBlockX, kTsdfBlockY), 0, stream, a);
  if (int rc = launch_check(h, "tsdf raycast")) return rc;
  return stage_counts(h, stream, d_totals, 1, d_counts, counts);
}

void pm_debug_tsdf_constants(int* lanes, int* waves) {
  if (lanes) *lanes = kTsdfLanes;
  if (waves) *waves = kTsdfWaves;
}

// ---- the volume's zero level set as one welded triangle mesh (pm_tsdf_mesh.hpp) ---------------------------------------------------
namespace {
size_t tsdf_mesh_spans(int nx, int ny, int nz) { return (((size_t)nx + kTsdfLanes - 1) / kTsdfLanes) * (size_t)ny * (size_t)nz; }

size_t tsdf_mesh_groups(size_t spans) { return (spans + kTsdfMeshGroup - 1) / kTsdfMeshGroup; }

// the totals, one word per span and one per group of spans for the vertices and for the triangles, one word and one byte per node
size_t tsdf_mesh_scratch_bytes(int nx, int ny, int nz) {
  const size_t nodes = (size_t)nx * (size_t)ny * (size_t)nz, spans = tsdf_mesh_spans(nx, ny, nz);
  return sizeof(int) * (kCountsHeader + 2 * tsdf_mesh_groups(spans) + 2 * spans + nodes) + nodes;
}
}  // namespace

int pm_tsdf_mesh(pm_handle* h, const pm_tsdf_volume* volume, const pm_tsdf_mesh_options* options, const void* d_voxels,
                 int vertex_capacity, int tri_capacity, float* d_xyz_out, float* d_normals_out, int32_t* d_tri_out, int* d_counts,
                 int* counts) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_tsdf_mesh";
  if (int rc = check_not_null(h, what, {{"volume", volume}, {"options", options}, {"d_voxels", d_voxels}})) return rc;
  if (const char* fault = tsdf_volume_fault(*volume)) {
    set_err(h, "%s: %s", what, fault);
    return PM_ERR_INVALID_ARG;
  }
  if (std::isnan(options->min_weight) || options->min_weight < 0.f) {
    set_err(h, "%s: min_weight must not be NaN or negative", what);
    return PM_ERR_INVALID_ARG;
  }
  if (vertex_capacity < 0 || tri_capacity < 0) {
    set_err(h, "%s: %s %d must be >= 0", what, vertex_capacity < 0 ? "vertex_capacity" : "tri_capacity",
            vertex_capacity < 0 ? vertex_capacity : tri_capacity);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_tsdf_size(h, what, *volume)) return rc;
  const int nx = volume->nx, ny = volume->ny, nz = volume->nz;
  const size_t nodes = tsdf_voxels(*volume);
  const size_t cells = (size_t)(nx - 1) * (size_t)(ny - 1) * (size_t)(nz - 1);
  if (7 * nodes > (size_t)INT32_MAX || kTsdfMeshMaxCellTriangles * cells > (size_t)INT32_MAX) {
    set_err(h, "%s: the %dx%dx%d volume has more than 2^31 - 1 possible vertices or triangles", what, nx, ny, nz);
    return PM_ERR_SIZE;
  }
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  const size_t spans = tsdf_mesh_spans(nx, ny, nz);  // <= nodes: far below 2^31
  PM_HIP(h, st->tsdf_mesh_buf.reserve(tsdf_mesh_scratch_bytes(nx, ny, nz), stream));
  int* d_totals = st->tsdf_mesh_buf.get();
  const bool want_vertices = vertex_capacity > 0 && (d_xyz_out || d_normals_out);
  const bool want_tris = tri_capacity > 0 && d_tri_out;
  TsdfMeshArgs a = {};
  a.grid = tsdf_grid(*volume);
  a.min_weight = options->min_weight;
  a.x_spans = (nx + kTsdfLanes - 1) / kTsdfLanes;
  a.voxels = static_cast<const TsdfVoxel*>(d_voxels);
  const size_t groups = tsdf_mesh_groups(spans);
  a.vertex_groups = d_totals + kCountsHeader;
  a.tri_groups = a.vertex_groups + groups;
  a.vertex_spans = a.tri_groups + groups;
  a.tri_spans = a.vertex_spans + spans;
  a.info = reinterpret_cast<uint32_t*>(a.tri_spans + spans);
  a.flags = reinterpret_cast<uint8_t*>(a.info + nodes);
  a.xyz_out = d_xyz_out, a.normals_out = d_normals_out, a.tri_out = d_tri_out;
  a.vertex_capacity = want_vertices ? vertex_capacity : 0, a.tri_capacity = want_tris ? tri_capacity : 0;
  const dim3 grid((unsigned)((spans + kTsdfBlockY - 1) / kTsdfBlockY)), block(kTsdfBlockX, kTsdfBlockY);
  const unsigned n_spans = (unsigned)spans;
  hipLaunchKernelGGL(k_tsdf_mesh_flags, grid, block, 0, stream, a, n_spans);
  hipLaunchKernelGGL(k_tsdf_mesh_count, grid, block, 0, stream, a, n_spans);
  hipLaunchKernelGGL(k_tsdf_mesh_span_offsets, dim3((unsigned)groups), dim3(kTsdfMeshGroup), 0, stream, a, n_spans);
  hipLaunchKernelGGL(k_cloud_offsets, dim3(1), dim3(kCloudScanThreads), 0, stream, a.vertex_groups, (int)groups, d_totals, d_counts);
  hipLaunchKernelGGL(k_cloud_offsets, dim3(1), dim3(kCloudScanThreads), 0, stream, a.tri_groups, (int)groups, d_totals + 1,
                     d_counts ? d_counts + 1 : nullptr);
  if (want_vertices) hipLaunchKernelGGL(k_tsdf_mesh_vertices, grid, block, 0, stream, a, n_spans);
  if (want_tris) hipLaunchKernelGGL(k_tsdf_mesh_triangles, grid, block, 0, stream, a, n_spans);
  if (int rc = launch_check(h, "tsdf mesh")) return rc;
  return stage_counts(h, stream, d_totals, 2, nullptr, counts);  // k_cloud_offsets wrote d_counts
}

void pm_debug_tsdf_mesh_table(uint8_t* counts, uint8_t* codes) {
  for (unsigned pattern = 0; pattern < 256; ++pattern) {
    int n = 0;
    uint8_t* row = codes ? codes + 3 * kTsdfMeshMaxCellTriangles * pattern : nullptr;
    for (int m = 0; row && m < 3 * kTsdfMeshMaxCellTriangles; ++m) row[m] = 0xff;
    tsdf_mesh_cell_triangles(pattern, [&](unsigned c0, unsigned c1, unsigned c2) {
      if (row) row[3 * n] = (uint8_t)c0, row[3 * n + 1] = (uint8_t)c1, row[3 * n + 2] = (uint8_t)c2;
      ++n;
    });
    if (counts) counts[pattern] = (uint8_t)n;
  }
}

size_t pm_debug_tsdf_mesh_scratch_bytes(int nx, int ny, int nz) {
  return nx < 1 || ny < 1 || nz < 1 ? 0 : tsdf_mesh_scratch_bytes(nx, ny, nz);
}

// ---- colour in the model: a colour volume beside the distance volume, integrated with it and gathered back (pm_tsdf_color.hpp) --
namespace {
// what the two gathers check of their options
int check_tsdf_color_sample(pm_handle* h, const char* what, const pm_tsdf_color_sample_options& o) {
  if (std::isnan(o.min_weight) || o.min_weight < 0.f) {
    set_err(h, "%s: min_weight must not be NaN or negative", what);
    return PM_ERR_INVALID_ARG;
  }
  if (!std::isfinite(o.byte_scale) || !(o.byte_scale > 0.f)) {
    set_err(h, "%s: byte_scale must be finite and > 0", what);
    return PM_ERR_INVALID_ARG;
  }
  return PM_OK;
}

TsdfColorSampler tsdf_color_sampler(const pm_tsdf_volume& v, const pm_tsdf_color_sample_options& o, const void* d_colors,
                                    float* d_bgr_out, uint8_t* d_bgr8_out, int* d_totals) {
  return TsdfColorSampler{tsdf_grid(v), o.min_weight, o.byte_scale, static_cast<const TsdfColor*>(d_colors), d_bgr_out, d_bgr8_out,
                          d_totals};
}
}  // namespace

size_t pm_tsdf_color_bytes(const pm_tsdf_volume* volume) {
  if (!volume || tsdf_volume_fault(*volume)) return 0;
  return tsdf_voxels(*volume) * sizeof(TsdfColor);
}

int pm_tsdf_color_clear(pm_handle* h, const pm_tsdf_volume* volume, void* d_colors) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_tsdf_color_clear";
  if (int rc = check_not_null(h, what, {{"volume", volume}, {"d_colors", d_colors}})) return rc;
  if (const char* fault = tsdf_volume_fault(*volume)) {
    set_err(h, "%s: %s", what, fault);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_tsdf_size(h, what, *volume)) return rc;
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  PM_HIP(h, hipMemsetAsync(d_colors, 0, tsdf_voxels(*volume) * sizeof(TsdfColor), pm_internal::stream(h)));
  return PM_OK;
}

int pm_tsdf_integrate_color(pm_handle* h, const pm_cloud_camera* camera, const pm_tsdf_volume* volume, const pm_motion* pose,
                            const pm_tsdf_color_options* options, const float* d_disp, const float* d_weight,
                            const uint8_t* d_bgr8, const float* d_bgr, int rows, int cols, void* d_voxels, void* d_colors,
                            int* d_counts, int* counts) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_tsdf_integrate_color";
  if (int rc = check_tsdf_integrate(h, what, camera, volume, pose, options, d_disp, rows, cols, d_voxels)) return rc;
  if (int rc = check_not_null(h, what, {{"d_colors", d_colors}})) return rc;
  if ((d_bgr8 != nullptr) == (d_bgr != nullptr)) {
    set_err(h, "%s: exactly one of d_bgr8 and d_bgr must be given (%s)", what, d_bgr8 ? "both are" : "neither is");
    return PM_ERR_INVALID_ARG;
  }
  if (!(options->band > 0.f && options->band <= 1.f)) {
    set_err(h, "%s: band must lie in (0, 1]", what);
    return PM_ERR_INVALID_ARG;
  }
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  int* d_totals = nullptr;
  if (int rc = counts_scratch(h, st->tsdf_counts, stream, &d_totals)) return rc;
  TsdfIntegrateColorArgs a = {};
  a.base.cam = cloud_cam(*camera);
  a.base.grid = tsdf_grid(*volume);
  set_motion(a.base.R, a.base.t, pose);
  a.base.min_disp = options->min_disp, a.base.max_range = options->max_range;
  a.base.disp = d_disp, a.base.weight = d_weight, a.base.rows = rows, a.base.cols = cols;
  a.base.voxels = static_cast<TsdfVoxel*>(d_voxels), a.base.counts = d_totals;
  a.bandw = (double)options->band * volume->trunc;
  a.bgr8 = d_bgr8, a.bgr = d_bgr, a.colors = static_cast<TsdfColor*>(d_colors);
  hipLaunchKernelGGL(k_tsdf_integrate_color, tsdf_span_grid(*volume), dim3(kTsdfBlockX, kTsdfBlockY), 0, stream, a);
  if (int rc = launch_check(h, "tsdf integrate color")) return rc;
  return stage_counts(h, stream, d_totals, 3, d_counts, counts);
}

int pm_tsdf_color_map(pm_handle* h, const pm_cloud_camera* camera, const pm_tsdf_volume* volume, const pm_motion* pose,
                      const pm_tsdf_color_sample_options* options, const void* d_colors, const float* d_disp, int rows, int cols,
                      float* d_bgr_out, uint8_t* d_bgr8_out, int* d_counts, int* counts) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_tsdf_color_map";
  if (int rc = check_tsdf_common(h, what, camera, volume, pose, options, d_colors, "d_colors")) return rc;
  if (int rc = check_not_null(h, what, {{"d_disp", d_disp}})) return rc;
  if (int rc = check_tsdf_color_sample(h, what, *options)) return rc;
  if (int rc = check_cloud_shape(h, what, rows, cols)) return rc;
  if (int rc = check_any_output(h, what, {d_bgr_out, d_bgr8_out, d_counts, counts}, "d_bgr_out, d_bgr8_out, d_counts and counts"))
    return rc;
  if (int rc = check_tsdf_size(h, what, *volume)) return rc;
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  int* d_totals = nullptr;
  if (int rc = counts_scratch(h, st->tsdf_counts, stream, &d_totals)) return rc;
  TsdfColorMapArgs a = {};
  a.s = tsdf_color_sampler(*volume, *options, d_colors, d_bgr_out, d_bgr8_out, d_totals);
  a.cam = cloud_cam(*camera);
  motion_inverse(pose->R, pose->t, a.Ri, a.c);  // in binary64, as pm_tsdf_raycast forms it
  a.disp = d_disp, a.rows = rows, a.cols = cols;
  const dim3 grid((unsigned)((cols + kTsdfLanes - 1) / kTsdfLanes), (unsigned)((rows + kTsdfBlockY - 1) / kTsdfBlockY));
  hipLaunchKernelGGL(k_tsdf_color_map, grid, dim3(kTsdfBlockX, kTsdfBlockY), 0, stream, a);
  if (int rc = launch_check(h, "tsdf color map")) return rc;
  return stage_counts(h, stream, d_totals, 1, d_counts, counts);
}

int pm_tsdf_color_points(pm_handle* h, const pm_tsdf_volume* volume, const pm_tsdf_color_sample_options* options,
                         const void* d_colors, const float* d_xyz, int n, const int* d_n, float* d_bgr_out, uint8_t* d_bgr8_out,
                         int* d_counts, int* counts) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_tsdf_color_points";
  if (int rc = check_not_null(h, what, {{"volume", volume}, {"options", options}, {"d_colors", d_colors}, {"d_xyz", d_xyz}}))
    return rc;
  if (const char* fault = tsdf_volume_fault(*volume)) {
    set_err(h, "%s: %s", what, fault);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_tsdf_color_sample(h, what, *options)) return rc;
  if (n < 0) {
    set_err(h, "%s: n %d must be >= 0", what, n);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_any_output(h, what, {d_bgr_out, d_bgr8_out, d_counts, counts}, "d_bgr_out, d_bgr8_out, d_counts and counts"))
    return rc;
  if (n > INT32_MAX / 3) {
    set_err(h, "%s: n %d exceeds (2^31 - 1) / 3 points", what, n);
    return PM_ERR_SIZE;
  }
  if (int rc = check_tsdf_size(h, what, *volume)) return rc;
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  int* d_totals = nullptr;
  if (int rc = counts_scratch(h, st->tsdf_counts, stream, &d_totals)) return rc;
  if (n > 0) {
    TsdfColorPointsArgs a = {};
    a.s = tsdf_color_sampler(*volume, *options, d_colors, d_bgr_out, d_bgr8_out, d_totals);
    a.xyz = d_xyz, a.n = n, a.d_n = d_n;
    const unsigned per_block = kTsdfBlockX * kTsdfBlockY;
    hipLaunchKernelGGL(k_tsdf_color_points, dim3(((unsigned)n + per_block - 1) / per_block), dim3(kTsdfBlockX, kTsdfBlockY), 0,
                       stream, a);
    if (int rc = launch_check(h, "tsdf color points")) return rc;
  }
  return stage_counts(h, stream, d_totals, 1, d_counts, counts);
}

void pm_debug_tsdf_color_constants(int* record_bytes, int* lanes, int* waves) {
  if (record_bytes) *record_bytes = (int)sizeof(TsdfColor);
  if (lanes) *lanes = kTsdfLanes;
  if (waves) *waves = kTsdfWaves;
}

// ---- camera motion between two frames: features of the old left image tracked into the new one (pm_track.hpp) ----------------
namespace {
// what pm_track_features and pm_estimate_motion are both given
struct TrackInputs {
  const pm_cloud_camera* camera;
  const pm_track_options* options;
  const pm_motion* guess;  // null: the identity
  const uint8_t* left_old;
  const float* disp_old;
  const uint8_t* left_new;
  int rows, cols;
};

// what run_track leaves behind: where the records and the number of features are on the device, and the stream
struct TrackRun {
  pm_track* records;
  const int* d_total;
  hipStream_t stream;
};

// The checks of everything but the outputs, in a fixed order.
int check_track(pm_handle* h, const char* what, const TrackInputs& in) {
  const pm_track_options* o = in.options;
  if (int rc = check_cloud_camera(h, what, in.camera)) return rc;
  if (int rc = check_not_null(h, what, {{"options", o}, {"d_left_old", in.left_old}, {"d_disp_old", in.disp_old},
                                        {"d_left_new", in.left_new}}))
    return rc;
  if (in.guess)
    if (int rc = check_motion(h, what, *in.guess, "the guess")) return rc;
  if (o->cell < kTrackMinCell || o->cell > kTrackMaxCell) {
    set_err(h, "%s: cell %d outside %d..%d", what, o->cell, kTrackMinCell, kTrackMaxCell);
    return PM_ERR_INVALID_ARG;
  }
  if (o->patch_radius < 1 || o->patch_radius > kTrackMaxPatch) {
    set_err(h, "%s: patch_radius %d outside 1..%d", what, o->patch_radius, kTrackMaxPatch);
    return PM_ERR_INVALID_ARG;
  }
  if (o->search_radius < 0 || o->search_radius > kTrackMaxSearch) {
    set_err(h, "%s: search_radius %d outside 0..%d", what, o->search_radius, kTrackMaxSearch);
    return PM_ERR_INVALID_ARG;
  }
  if (o->min_score < 1) {
    set_err(h, "%s: min_score %lld must be >= 1", what, (long long)o->min_score);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_disp_limits(h, what, o->min_disp, o->max_disp)) return rc;
  if (o->max_sad < 0 || o->min_gap < 0) {
    set_err(h, "%s: %s must be >= 0", what, o->max_sad < 0 ? "max_sad" : "min_gap");
    return PM_ERR_INVALID_ARG;
  }
  return check_cloud_shape(h, what, in.rows, in.cols);
}

int track_cells(int n, int cell) { return (n + cell - 1) / cell; }

// The three launches.  Scratch: kCountsHeader words, the per-cell results, the feature list and, with `own_records`, one
// record per cell behind them, which then take the place of d_tracks and capacity.
int run_track(pm_handle* h, const char* what, const TrackInputs& in, int capacity, pm_track* d_tracks, int* d_count,
              bool own_records, TrackRun* run) {
  const pm_track_options* o = in.options;
  const int rows = in.rows, cols = in.cols;
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  const int ncx = track_cells(cols, o->cell), ncy = track_cells(rows, o->cell);
  const size_t cells = (size_t)ncx * ncy;  // <= rows * cols / 64 + ...: far below 2^31 (check_cloud_shape)
  const size_t words = kCountsHeader + 2 * cells;
  PM_HIP(h, st->track_buf.reserve(sizeof(int) * words + (own_records ? sizeof(pm_track) * cells : 0), stream));
  int* base = st->track_buf.get();
  int* cell_best = base + kCountsHeader;
  int* feat = cell_best + cells;
  if (own_records) {
    d_tracks = reinterpret_cast<pm_track*>(base + words);
    capacity = (int)cells;
  }
  const TrackOpt opt = {o->cell, o->patch_radius, o->search_radius, (long long)o->min_score, o->min_disp, o->max_disp,
                        o->max_sad,  o->min_gap};
  hipLaunchKernelGGL(k_track_select, dim3((unsigned)ncx, (unsigned)ncy), dim3(kTrackBlock), 0, stream,
                     TrackSelectArgs{opt, in.left_old, in.disp_old, rows, cols, cell_best});
  hipLaunchKernelGGL(k_track_compact, dim3(1), dim3(kTrackCompactThreads), 0, stream, (const int*)cell_best, (int)cells, feat,
                     base, d_count);
  const size_t blocks = cells < (size_t)capacity ? cells : (size_t)capacity;
  if (blocks > 0 && d_tracks) {
    TrackMatchArgs a = {};
    a.opt = opt, a.cam = cloud_cam(*in.camera);
    set_motion(a.R, a.t, in.guess);
    a.old = in.left_old, a.disp = in.disp_old, a.img = in.left_new, a.rows = rows, a.cols = cols;
    a.feat = feat, a.total = base, a.tracks = d_tracks;
    hipLaunchKernelGGL(k_track_match, dim3((unsigned)blocks), dim3(kTrackBlock), 0, stream, a);
  }
  if (int rc = launch_check(h, "track features")) return rc;
  *run = TrackRun{d_tracks, base, stream};
  return PM_OK;
}
}  // namespace

int pm_track_features(pm_handle* h, const pm_cloud_camera* camera, const pm_track_options* options, const pm_motion* guess,
                      const uint8_t* d_left_old, const float* d_disp_old, const uint8_t* d_left_new, int rows, int cols,
                      int capacity, pm_track* d_tracks, int* d_count, int* count) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_track_features";
  const TrackInputs in = {camera, options, guess, d_left_old, d_disp_old, d_left_new, rows, cols};
  if (int rc = check_track(h, what, in)) return rc;
  if (capacity < 0) {
    set_err(h, "%s: capacity %d must be >= 0", what, capacity);
    return PM_ERR_INVALID_ARG;
  }
  if (capacity > 0 && !d_tracks) {
    set_err(h, "%s: null d_tracks with capacity %d", what, capacity);
    return PM_ERR_INVALID_ARG;
  }
  if (capacity == 0 && !d_count && !count) {
    set_err(h, "%s: no output: capacity is 0, d_count and count are null", what);
    return PM_ERR_INVALID_ARG;
  }
  TrackRun run = {};
  if (int rc = run_track(h, what, in, capacity, d_tracks, d_count, false, &run)) return rc;
  return stage_counts(h, run.stream, run.d_total, 1, nullptr, count);  // k_track_compact wrote d_count
}

int pm_estimate_motion(pm_handle* h, const pm_cloud_camera* camera, const pm_track_options* track_options,
                       const pm_solve_options* solve_options, const pm_motion* guess, const uint8_t* d_left_old,
                       const float* d_disp_old, const uint8_t* d_left_new, int rows, int cols, pm_motion* out,
                       pm_motion_info* info) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_estimate_motion";
  const TrackInputs in = {camera, track_options, guess, d_left_old, d_disp_old, d_left_new, rows, cols};
  if (int rc = check_track(h, what, in)) return rc;
  const pm_solve_options* s = solve_options;
  if (int rc = check_not_null(h, what, {{"solve_options", s}})) return rc;
  if (s->iterations < 1 || s->iterations > 50) {
    set_err(h, "%s: iterations %d outside 1..50", what, s->iterations);
    return PM_ERR_INVALID_ARG;
  }
  if (!(s->huber_px > 0.0) || !(s->epsilon >= 0.0) || !(s->inlier_px > 0.0)) {
    set_err(h, "%s: %s and not NaN", what,
            !(s->huber_px > 0.0) ? "huber_px must be > 0" : !(s->epsilon >= 0.0) ? "epsilon must be >= 0" : "inlier_px must be > 0");
    return PM_ERR_INVALID_ARG;
  }
  if (s->min_inliers < 6) {
    set_err(h, "%s: min_inliers %d must be >= 6", what, s->min_inliers);
    return PM_ERR_INVALID_ARG;
  }
  if (!out && !info) {
    set_err(h, "%s: no output: out and info are null", what);
    return PM_ERR_INVALID_ARG;
  }
  TrackRun run = {};
  if (int rc = run_track(h, what, in, 0, nullptr, nullptr, true, &run)) return rc;
  int n = 0;
  if (int rc = stage_counts(h, run.stream, run.d_total, 1, nullptr, &n)) return rc;
  std::vector<pm_track> tracks;
  try {
    tracks.resize((size_t)n);
  } catch (const std::bad_alloc&) {
    set_err(h, "%s: out of host memory for %d records", what, n);
    return PM_ERR_NOMEM;
  }
  if (n > 0) {
    PM_HIP(h, hipMemcpyAsync(tracks.data(), run.records, sizeof(pm_track) * (size_t)n, hipMemcpyDeviceToHost, run.stream));
    PM_HIP(h, hipStreamSynchronize(run.stream));
  }
  const int rc = pm_solve_motion(camera, s, tracks.data(), n, guess, out, info);
  if (rc != PM_OK) set_err(h, "%s: pm_solve_motion refused its arguments", what);
  return rc;
}

// ---- dense alignment: a new map registered against the model's map and normals (pm_align.hpp) ---------------------------------
namespace {
constexpr size_t kAlignRecordSlot = 256;  // the record in front of the row sums, which stay 16-byte aligned behind it
static_assert(sizeof(pm_align_sums) <= kAlignRecordSlot, "the record fits its slot");

size_t align_scratch_bytes(int rows) { return kAlignRecordSlot + sizeof(double) * kAlignTerms * (size_t)rows; }

// what pm_align_evaluate and pm_align_disparity are both given
struct AlignInputs {
  const pm_cloud_camera* camera;
  const pm_align_options* options;
  const pm_motion* motion;  // null: the identity
  const float* disp_model;
  const float* normals_model;
  const float* disp_new;
  int rows, cols;
};

// The checks of everything but the outputs, in a fixed order; `whose`: the motion as the message names it.
int check_align(pm_handle* h, const char* what, const AlignInputs& in, const char* whose) {
  const pm_align_options* o = in.options;
  if (int rc = check_cloud_camera(h, what, in.camera)) return rc;
  if (int rc = check_not_null(h, what, {{"options", o}, {"d_disp_model", in.disp_model}, {"d_normals_model", in.normals_model},
                                        {"d_disp_new", in.disp_new}}))
    return rc;
  if (in.motion)
    if (int rc = check_motion(h, what, *in.motion, whose)) return rc;
  if (std::isnan(o->min_disp)) {
    set_err(h, "%s: min_disp must not be NaN", what);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_max_diff(h, what, o->max_diff)) return rc;
  if (!(o->huber_px > 0.0) || !(o->epsilon >= 0.0)) {
    set_err(h, "%s: %s and not NaN", what, !(o->huber_px > 0.0) ? "huber_px must be > 0" : "epsilon must be >= 0");
    return PM_ERR_INVALID_ARG;
  }
  if (o->iterations < 1 || o->iterations > 50) {
    set_err(h, "%s: iterations %d outside 1..50", what, o->iterations);
    return PM_ERR_INVALID_ARG;
  }
  if (o->min_used < 6) {
    set_err(h, "%s: min_used %d must be >= 6", what, o->min_used);
    return PM_ERR_INVALID_ARG;
  }
  return check_cloud_shape(h, what, in.rows, in.cols);
}

// One evaluation behind the checks: the 16-byte memset of the counts and the two launches.  *d_record: the handle's record.
int run_align(pm_handle* h, const char* what, const AlignInputs& in, const pm_motion* motion, uint8_t* d_class_out,
              float* d_residual_out, pm_align_sums* d_sums, ImagingState** state, hipStream_t* stream_out,
              pm_align_sums** d_record) {
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  PM_HIP(h, st->align_buf.reserve(align_scratch_bytes(in.rows), stream));
  if (!st->align_host.base()) PM_HIP(h, st->align_host.alloc(sizeof(pm_align_sums)));
  pm_align_sums* record = reinterpret_cast<pm_align_sums*>(st->align_buf.get());
  AlignArgs a = {};
  a.cam = cloud_cam(*in.camera);
  set_motion(a.R, a.t, motion);
  a.min_disp = in.options->min_disp, a.max_diff = in.options->max_diff, a.huber_px = in.options->huber_px;
  a.disp_model = in.disp_model, a.normals_model = in.normals_model, a.disp_new = in.disp_new;
  a.rows = in.rows, a.cols = in.cols;
  a.class_out = d_class_out, a.residual_out = d_residual_out;
  a.row_sums = reinterpret_cast<double*>(st->align_buf.get() + kAlignRecordSlot);
  a.counts = &record->n_model;
  PM_HIP(h, hipMemsetAsync(a.counts, 0, 4 * sizeof(int), stream));
  hipLaunchKernelGGL(k_align_rows, dim3(align_row_blocks(in.rows)), dim3(kAlignBlockX, kAlignBlockY), 0, stream, a);
  hipLaunchKernelGGL(k_align_finish, dim3(1), dim3(kAlignLanes), 0, stream, (const double*)a.row_sums, in.rows,
                     (const int*)a.counts, record, d_sums);
  if (int rc = launch_check(h, "align")) return rc;
  *state = st, *stream_out = stream, *d_record = record;
  return PM_OK;
}

// The handle's record through its page-locked memory into *sums; the copy has landed when this returns.
int align_download(pm_handle* h, ImagingState* st, hipStream_t stream, const pm_align_sums* d_record, pm_align_sums* sums) {
  PM_HIP(h, hipMemcpyAsync(st->align_host.base(), d_record, sizeof(pm_align_sums), hipMemcpyDeviceToHost, stream));
  PM_HIP(h, hipStreamSynchronize(stream));
  std::memcpy(sums, st->align_host.base(), sizeof(pm_align_sums));
  return PM_OK;
}

// The Gauss-Newton loop of pm_align_disparity and pm_align_color_disparity: record(m, &sums) gives the normal equations under m,
// pm_align_step solves and updates; it stops where a factorisation fails, after the update whose largest |delta_i| is below
// epsilon, or after `iterations` updates.  Behind it, one more record under the motion reached is in *sums.
template <typename Record>
int align_iterate(const pm_align_options& o, pm_motion* m, bool* failed, int* done, pm_align_sums* sums, Record record) {
  for (int it = 0; it < o.iterations; ++it) {
    if (int rc = record(*m, sums)) return rc;
    double delta[6];
    int factorised = 0;
    pm_align_step(sums, m, m, delta, &factorised);
    if (!factorised) {
      *failed = true;
      break;
    }
    ++*done;
    double biggest = 0.0;
    for (double v : delta) biggest = std::fabs(v) > biggest ? std::fabs(v) : biggest;
    if (biggest < o.epsilon) break;
  }
  return record(*m, sums);
}
}  // namespace

int pm_align_evaluate(pm_handle* h, const pm_cloud_camera* camera, const pm_align_options* options, const pm_motion* motion,
                      const float* d_disp_model, const float* d_normals_model, const float* d_disp_new, int rows, int cols,
                      uint8_t* d_class_out, float* d_residual_out, pm_align_sums* d_sums, pm_align_sums* sums) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_align_evaluate";
  const AlignInputs in = {camera, options, motion, d_disp_model, d_normals_model, d_disp_new, rows, cols};
  if (int rc = check_align(h, what, in, "the motion")) return rc;
  if (int rc = check_any_output(h, what, {d_class_out, d_residual_out, d_sums, sums}, "d_class_out, d_residual_out, d_sums and sums"))
    return rc;
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  pm_align_sums* d_record = nullptr;
  if (int rc = run_align(h, what, in, motion, d_class_out, d_residual_out, d_sums, &st, &stream, &d_record)) return rc;
  return sums ? align_download(h, st, stream, d_record, sums) : PM_OK;
}

int pm_align_disparity(pm_handle* h, const pm_cloud_camera* camera, const pm_align_options* options, const pm_motion* guess,
                       const float* d_disp_model, const float* d_normals_model, const float* d_disp_new, int rows, int cols,
                       pm_motion* out, pm_align_info* info) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_align_disparity";
  const AlignInputs in = {camera, options, guess, d_disp_model, d_normals_model, d_disp_new, rows, cols};
  if (int rc = check_align(h, what, in, "the guess")) return rc;
  if (int rc = check_any_output(h, what, {out, info}, "out and info")) return rc;
  pm_motion start;
  set_motion(start.R, start.t, guess);
  pm_motion m = start;
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  pm_align_sums* d_record = nullptr;
  pm_align_sums sums;
  const auto record = [&](const pm_motion& at, pm_align_sums* into) -> int {
    if (int rc = run_align(h, what, in, &at, nullptr, nullptr, nullptr, &st, &stream, &d_record)) return rc;
    return align_download(h, st, stream, d_record, into);
  };
  bool failed = false;
  int done = 0;
  if (int rc = align_iterate(*options, &m, &failed, &done, &sums, record)) return rc;
  const bool valid = !failed && sums.n_used >= options->min_used;
  if (out) *out = valid ? m : start;
  if (info) {
    info->valid = valid ? 1 : 0;
    info->n_model = sums.n_model, info->n_gate = sums.n_gate, info->n_used = sums.n_used;
    info->iterations = done;
    info->rms_px = sums.n_used ? std::sqrt(sums.rr / (double)sums.n_used) : 0.0;
    for (int i = 0; i < 21; ++i) info->H[i] = sums.H[i];
  }
  return PM_OK;
}

void pm_debug_align_constants(int* lanes, int* waves) {
  if (lanes) *lanes = kAlignLanes;
  if (waves) *waves = kAlignWaves;
}

size_t pm_debug_align_scratch_bytes(int rows) { return rows < 1 ? 0 : align_scratch_bytes(rows); }

// ---- the photometric term of the dense alignment: lumas, one evaluation, the blended loop (pm_align_photo.hpp) ------------------
namespace {
// a second record slot and a second run of row sums, then the two luma planes of pm_align_color_disparity
size_t align_photo_scratch_bytes(int rows, int cols) {
  return align_scratch_bytes(rows) + 2 * sizeof(float) * (size_t)rows * (size_t)cols;
}

int check_one_image(pm_handle* h, const char* what, const uint8_t* d_bgr8, const float* d_bgr, const char* name8, const char* name) {
  if ((d_bgr8 != nullptr) == (d_bgr != nullptr)) {
    set_err(h, "%s: exactly one of %s and %s must be given (%s)", what, name8, name, d_bgr8 ? "both are" : "neither is");
    return PM_ERR_INVALID_ARG;
  }
  return PM_OK;
}

// One luma plane behind the checks: one launch.
int run_luma(pm_handle* h, hipStream_t stream, const uint8_t* d_bgr8, const float* d_bgr, int rows, int cols, int zero_is_absent,
             float* d_luma_out) {
  const LumaArgs a = {d_bgr8, d_bgr, rows, cols, zero_is_absent, d_luma_out};
  const LumaBlocks blocks = luma_blocks(rows, cols);
  hipLaunchKernelGGL(k_bgr_luma, dim3(blocks.x, blocks.y), dim3(kAlignBlockX, kAlignBlockY), 0, stream, a);
  return launch_check(h, "bgr luma");
}

// what pm_align_photo_evaluate is given and pm_align_color_disparity makes
struct AlignPhotoInputs {
  const pm_cloud_camera* camera;
  float min_disp, max_diff;
  double huber_levels;
  const float* disp_model;
  const float* luma_model;
  const float* disp_new;
  const float* luma_new;
  int rows, cols;
};

int check_huber_levels(pm_handle* h, const char* what, double huber_levels) {
  if (!(huber_levels > 0.0)) {
    set_err(h, "%s: huber_levels must be > 0 and not NaN", what);
    return PM_ERR_INVALID_ARG;
  }
  return PM_OK;
}

// One photometric evaluation behind the checks, as run_align: the 16-byte memset of the counts and the two launches.
int run_align_photo(pm_handle* h, const char* what, const AlignPhotoInputs& in, const pm_motion* motion, uint8_t* d_class_out,
                    float* d_residual_out, pm_align_sums* d_sums, ImagingState** state, hipStream_t* stream_out,
                    pm_align_sums** d_record) {
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  PM_HIP(h, st->align_photo_buf.reserve(align_photo_scratch_bytes(in.rows, in.cols), stream));
  if (!st->align_photo_host.base()) PM_HIP(h, st->align_photo_host.alloc(sizeof(pm_align_sums)));
  pm_align_sums* record = reinterpret_cast<pm_align_sums*>(st->align_photo_buf.get());
  AlignPhotoArgs a = {};
  a.cam = cloud_cam(*in.camera);
  set_motion(a.R, a.t, motion);
  a.min_disp = in.min_disp, a.max_diff = in.max_diff, a.huber_levels = in.huber_levels;
  a.disp_model = in.disp_model, a.luma_model = in.luma_model, a.disp_new = in.disp_new, a.luma_new = in.luma_new;
  a.rows = in.rows, a.cols = in.cols;
  a.class_out = d_class_out, a.residual_out = d_residual_out;
  a.row_sums = reinterpret_cast<double*>(st->align_photo_buf.get() + kAlignRecordSlot);
  a.counts = &record->n_model;
  PM_HIP(h, hipMemsetAsync(a.counts, 0, 4 * sizeof(int), stream));
  hipLaunchKernelGGL(k_align_photo_rows, dim3(align_row_blocks(in.rows)), dim3(kAlignBlockX, kAlignBlockY), 0, stream, a);
  hipLaunchKernelGGL(k_align_finish, dim3(1), dim3(kAlignLanes), 0, stream, (const double*)a.row_sums, in.rows,
                     (const int*)a.counts, record, d_sums);
  if (int rc = launch_check(h, "align photo")) return rc;
  *state = st, *stream_out = stream, *d_record = record;
  return PM_OK;
}
}  // namespace

int pm_bgr_luma(pm_handle* h, const uint8_t* d_bgr8, const float* d_bgr, int rows, int cols, int zero_is_absent,
                float* d_luma_out) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_bgr_luma";
  if (int rc = check_one_image(h, what, d_bgr8, d_bgr, "d_bgr8", "d_bgr")) return rc;
  if (int rc = check_not_null(h, what, {{"d_luma_out", d_luma_out}})) return rc;
  if (int rc = check_cloud_shape(h, what, rows, cols)) return rc;
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  return run_luma(h, pm_internal::stream(h), d_bgr8, d_bgr, rows, cols, zero_is_absent, d_luma_out);
}

int pm_align_photo_evaluate(pm_handle* h, const pm_cloud_camera* camera, const pm_align_photo_options* options,
                            const pm_motion* motion, const float* d_disp_model, const float* d_luma_model, const float* d_disp_new,
                            const float* d_luma_new, int rows, int cols, uint8_t* d_class_out, float* d_residual_out,
                            pm_align_sums* d_sums, pm_align_sums* sums) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_align_photo_evaluate";
  if (int rc = check_cloud_camera(h, what, camera)) return rc;
  if (int rc = check_not_null(h, what, {{"options", options}, {"d_disp_model", d_disp_model}, {"d_luma_model", d_luma_model},
                                        {"d_disp_new", d_disp_new}, {"d_luma_new", d_luma_new}}))
    return rc;
  if (motion)
    if (int rc = check_motion(h, what, *motion, "the motion")) return rc;
  if (std::isnan(options->min_disp)) {
    set_err(h, "%s: min_disp must not be NaN", what);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_max_diff(h, what, options->max_diff)) return rc;
  if (int rc = check_huber_levels(h, what, options->huber_levels)) return rc;
  if (int rc = check_cloud_shape(h, what, rows, cols)) return rc;
  if (int rc = check_any_output(h, what, {d_class_out, d_residual_out, d_sums, sums}, "d_class_out, d_residual_out, d_sums and sums"))
    return rc;
  const AlignPhotoInputs in = {camera, options->min_disp, options->max_diff, options->huber_levels, d_disp_model, d_luma_model,
                               d_disp_new, d_luma_new, rows, cols};
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  pm_align_sums* d_record = nullptr;
  if (int rc = run_align_photo(h, what, in, motion, d_class_out, d_residual_out, d_sums, &st, &stream, &d_record)) return rc;
  if (!sums) return PM_OK;
  PM_HIP(h, hipMemcpyAsync(st->align_photo_host.base(), d_record, sizeof(pm_align_sums), hipMemcpyDeviceToHost, stream));
  PM_HIP(h, hipStreamSynchronize(stream));
  std::memcpy(sums, st->align_photo_host.base(), sizeof(pm_align_sums));
  return PM_OK;
}

int pm_align_color_disparity(pm_handle* h, const pm_cloud_camera* camera, const pm_align_color_options* options,
                             const pm_motion* guess, const float* d_disp_model, const float* d_normals_model,
                             const float* d_bgr_model, const float* d_disp_new, const uint8_t* d_bgr8_new, const float* d_bgr_new,
                             int rows, int cols, pm_motion* out, pm_align_color_info* info) {
  if (!h) return PM_ERR_INVALID_ARG;
  const char* const what = "pm_align_color_disparity";
  const AlignInputs in = {camera, options ? &options->align : nullptr, guess, d_disp_model, d_normals_model, d_disp_new, rows, cols};
  if (int rc = check_align(h, what, in, "the guess")) return rc;
  if (int rc = check_any_output(h, what, {out, info}, "out and info")) return rc;
  if (int rc = check_not_null(h, what, {{"d_bgr_model", d_bgr_model}})) return rc;
  if (int rc = check_one_image(h, what, d_bgr8_new, d_bgr_new, "d_bgr8_new", "d_bgr_new")) return rc;
  if (int rc = check_huber_levels(h, what, options->huber_levels)) return rc;
  if (!(std::isfinite(options->lambda) && options->lambda >= 0.0)) {
    set_err(h, "%s: lambda must be finite and >= 0", what);
    return PM_ERR_INVALID_ARG;
  }
  ImagingState* st = nullptr;
  hipStream_t stream = nullptr;
  if (int rc = stage_begin(h, what, &st, &stream)) return rc;
  // the two luma planes, once per call, behind the record slot and the row sums of the evaluations below
  PM_HIP(h, st->align_photo_buf.reserve(align_photo_scratch_bytes(rows, cols), stream));
  float* luma_model = reinterpret_cast<float*>(st->align_photo_buf.get() + align_scratch_bytes(rows));
  float* luma_new = luma_model + (size_t)rows * cols;
  if (int rc = run_luma(h, stream, nullptr, d_bgr_model, rows, cols, 1, luma_model)) return rc;
  if (int rc = run_luma(h, stream, d_bgr8_new, d_bgr_new, rows, cols, 0, luma_new)) return rc;
  const AlignPhotoInputs photo_in = {camera, options->align.min_disp, options->align.max_diff, options->huber_levels, d_disp_model,
                                     luma_model, d_disp_new, luma_new, rows, cols};
  pm_motion start;
  set_motion(start.R, start.t, guess);
  pm_motion m = start;
  pm_align_sums geo, photo, sums;
  // one geometric and one photometric evaluation under the same motion, both records behind one synchronisation, blended
  const auto record = [&](const pm_motion& at, pm_align_sums* into) -> int {
    pm_align_sums *d_geo = nullptr, *d_photo = nullptr;
    if (int rc = run_align(h, what, in, &at, nullptr, nullptr, nullptr, &st, &stream, &d_geo)) return rc;
    if (int rc = run_align_photo(h, what, photo_in, &at, nullptr, nullptr, nullptr, &st, &stream, &d_photo)) return rc;
    PM_HIP(h, hipMemcpyAsync(st->align_host.base(), d_geo, sizeof(pm_align_sums), hipMemcpyDeviceToHost, stream));
    PM_HIP(h, hipMemcpyAsync(st->align_photo_host.base(), d_photo, sizeof(pm_align_sums), hipMemcpyDeviceToHost, stream));
    PM_HIP(h, hipStreamSynchronize(stream));
    std::memcpy(&geo, st->align_host.base(), sizeof geo);
    std::memcpy(&photo, st->align_photo_host.base(), sizeof photo);
    return pm_align_sums_blend(&geo, &photo, options->lambda, into);
  };
  bool failed = false;
  int done = 0;
  if (int rc = align_iterate(options->align, &m, &failed, &done, &sums, record)) return rc;
  const bool valid = !failed && geo.n_used + photo.n_used >= options->align.min_used;
  if (out) *out = valid ? m : start;
  if (info) {
    info->geo.valid = valid ? 1 : 0;
    info->geo.n_model = geo.n_model, info->geo.n_gate = geo.n_gate, info->geo.n_used = geo.n_used;
    info->geo.iterations = done;
    info->geo.rms_px = geo.n_used ? std::sqrt(geo.rr / (double)geo.n_used) : 0.0;
    for (int i = 0; i < 21; ++i) info->geo.H[i] = geo.H[i];
    info->n_photo_model = photo.n_model, info->n_photo_gate = photo.n_gate, info->n_photo_used = photo.n_used;
    info->rms_levels = photo.n_used ? std::sqrt(photo.rr / (double)photo.n_used) : 0.0;
    for (int i = 0; i < 21; ++i) info->H[i] = sums.H[i];
  }
  return PM_OK;
}

size_t pm_debug_align_photo_scratch_bytes(int rows, int cols) {
  return rows < 1 || cols < 1 ? 0 : align_photo_scratch_bytes(rows, cols);
}
