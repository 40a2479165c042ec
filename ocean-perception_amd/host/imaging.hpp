// imaging.hpp -- host-side C++ mirror of the bm::imaging functions on the rows either side of the stereo
// hot path, same names and signatures as the reference headers
//   src/vehicle/imaging/normalization.hpp:12,41   Normalize, NormalizeColorIlluminant
//   src/vehicle/imaging/illuminant.hpp:10-21      EstimateIlluminantGaussian, EstimateIlluminantRangeGuided
//   src/vehicle/imaging/fast_guided_filter.hpp:27 fastGuidedFilter (one-channel guide)
//   src/vehicle/imaging/backscatter.hpp:13,45     FindDarkFast, RemoveBackscatter
//   src/vehicle/imaging/attenuation.hpp:59        CorrectAttenuation
//   src/vehicle/vision_core/image_util.hpp:34     ComputeIntensity
//   src/vehicle/vision_core/image_util.cpp:25     CastImage3bTo3f
// over the C ABI of pm/imaging.h.  Host images in, host images out: each call uploads, runs the device
// kernels and downloads (callers that keep images on the device use the C ABI directly).
// No HIP header, no OpenCV, no Eigen: Image3f is bm::core::Image<Vec3f> (interleaved BGR like cv::Vec3f),
// Vector3f / Vector12f are std::array.  The functions run on a process-wide context (device 0 unless
// SetDevice() is called first) and throw std::runtime_error when no GPU is usable -- there is no CPU path.
#pragma once

#include <array>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "patchmatch_gpu.hpp"
#include "pm/imaging.h"

namespace bm {
namespace core {
struct Vec3f {
  float v[3];
  float& operator()(int i) { return v[i]; }
  float operator()(int i) const { return v[i]; }
};
struct Vec3b {
  uint8_t v[3];
};
typedef Image<Vec3f> Image3f;
typedef Image<Vec3b> Image3b;
typedef std::array<float, 3> Vector3f;
typedef std::array<float, 12> Vector12f;
}  // namespace core

namespace imaging {
using namespace core;

// Device used by the free functions below; call before the first of them (default 0).
void SetDevice(int device);

Image3f CastImage3bTo3f(const Image3b& im);
Image1f ComputeIntensity(const Image3f& bgr);
Image3f EstimateIlluminantGaussian(const Image3f& bgr, int ksizeX, int ksizeY, double sigmaX, double sigmaY);
Image3f EstimateIlluminantRangeGuided(const Image3f& bgr, const Image1f& range, int r, double eps, int s);
// fastGuidedFilter(I, p, r, eps, s) with a one-channel float guide I; p has one or three channels.  (The reference
// takes cv::Mat and a depth argument; the colour guide, which nothing in the reference calls, is not provided.)
Image1f fastGuidedFilter(const Image1f& guide, const Image1f& src, int r, double eps, int s = 1);
Image3f fastGuidedFilter(const Image1f& guide, const Image3f& src, int r, double eps, int s = 1);
Image3f Normalize(const Image3f& bgr);
Image3f NormalizeColorIlluminant(const Image3f bgr);
float FindDarkFast(const Image1f& intensity, const Image1f& range, float percentile, Image1b& mask);
Image3f RemoveBackscatter(const Image3f& bgr, const Image1f& range, const Vector3f& B, const Vector3f& beta_B);
Image3f CorrectAttenuation(const Image3f& bgr, const Image1f& range, const Vector12f& X);

// Not in the reference as a function: the chain the reference's tests assemble by hand
// (test/imaging/enhance_test.cpp:69-73): 8-bit colour image -> the 8-bit gray image Match() consumes.
Image1b StereoReady(const Image3b& bgr);
// StereoCamera::DispToDepth (vision_core/stereo_camera.cpp:49-53) over a map; 0 where disp <= 0.
Image1f DispToDepth(const Image1f& disp, double fx, double baseline);

// Not in the reference, which warns "distortion_coefficients are nonzero, but we don't handle undistortion yet"
// (src/vehicle/params/yaml_parser.cpp:153): undistortion + rectification of a raw frame (pm/imaging.h, pm_rectify_u8).
struct CameraModel {  // radial-tangential, the entries of pm_camera
  double fx = 0, fy = 0, cx = 0, cy = 0, k1 = 0, k2 = 0, p1 = 0, p2 = 0, k3 = 0;
};
typedef pm_rectify_view RectifyView;
// Rectifying rotations and a common pinhole for a calibrated pair, X2 = R X1 + T (camera 1 = left; R row-major); returns
// the rectified baseline.  Host only: needs no GPU.  Throws std::invalid_argument where pm_stereo_rectify refuses.
double StereoRectify(const CameraModel& cam1, const CameraModel& cam2, const std::array<double, 9>& R,
                     const std::array<double, 3>& T, RectifyView* view1, RectifyView* view2);
// The raw image seen through `view`, rows x cols, pixels without a source 0; valid (255 / 0) where it is asked for.
Image1b Rectify(const Image1b& raw, const RectifyView& view, int rows, int cols, Image1b* valid = nullptr);
// The same for an interleaved 8-bit BGR frame (pm_rectify_bgr8): the three channels at one position, one mask.  Declared
// with the image classes themselves, not the Image1b alias, which a caller that compiles next to OpenCV sees as cv::Mat1b:
// the library exports this one signature whatever the caller includes.
core::Image<core::Vec3b> Rectify(const core::Image<core::Vec3b>& raw, const RectifyView& view, int rows, int cols,
                                 core::Image<uint8_t>* valid = nullptr);


// Not in the reference as functions: what its consumers of disparity do pixel by pixel on the host,
// LeftCamera().Backproject(pixel, DispToDepth(disp)) (src/vehicle/mesher/object_mesher.cpp:146-150,
// src/vehicle/vio/stereo_frontend.cpp:119, vision_core/pinhole_camera.cpp:41-45), for a whole map on the device
// (pm/imaging.h: pm_backproject, pm_point_cloud, pm_planes_normals; definition: tests/pointcloud_ref.py).  Declared with
// core::Image<...> itself, not the Image1f alias, for the reason given at the BGR Rectify overload.
struct StereoModel {  // the rectified left pinhole and the baseline: the entries of pm_cloud_camera
  double fx = 0, fy = 0, cx = 0, cy = 0, baseline = 0;
};
// organised points, (0, 0, 0) where disp is not > 0
core::Image<core::Vec3f> Backproject(const core::Image<float>& disp, const StereoModel& model);
struct CloudFilter {  // pm_cloud_filter
  float min_disp = 0.f;   // a pixel counts iff disp > 0 and disp >= min_disp
  float max_range = 0.f;  // > 0: and iff Z <= max_range; 0 = no limit
  int stride = 1;         // only pixels with x % stride == 0 and y % stride == 0
};
// The counted pixels in row-major order.  normals / bgr are empty where the matching input was not given.
struct PointCloud {
  std::vector<core::Vec3f> xyz;
  std::vector<core::Vec3f> normals;
  std::vector<core::Vec3b> bgr;
  std::vector<int32_t> index;  // y * cols + x
};
PointCloud MakePointCloud(const core::Image<float>& disp, const StereoModel& model, const CloudFilter& filter = CloudFilter(),
                          const core::Image<core::Vec3f>* normals = nullptr, const core::Image<core::Vec3b>* bgr = nullptr);
// PM_MODE_PLANES only: the organised unit normals of the left view, facing the camera, from the plane state the LAST
// Match() of `matcher` (rows x cols) left on the device -- the next Match() overwrites it.  disp_l: that Match()'s left map,
// whose zeros (the cross-check's mask) zero the normals; null = no mask.  Throws std::runtime_error where
// pm_planes_normals refuses (a scalar-mode matcher, no match yet, another size).
core::Image<core::Vec3f> PlaneNormals(pm::PatchmatchGpu& matcher, const StereoModel& model, int rows, int cols,
                                      const core::Image<float>* disp_l = nullptr);
// Any map, PM_MODE_SCALAR's included (it keeps no slopes): the organised unit normals of a least-squares plane fitted per
// pixel over a (2 radius + 1)^2 window (pm/imaging.h: pm_disparity_normals; definition: tests/normals_fit_ref.py), the input
// MakePointCloud takes as `normals`.  (0, 0, 0) where the map is not > 0 and where the fit has no support.
struct NormalsFit {  // pm_normals_fit
  int radius = 5;       // 1..7
  float max_diff = 1.f; // a tap counts iff its disparity is > 0 and within max_diff of the centre's (edge-aware)
  int min_support = 9;  // 3..(2 radius + 1)^2 counting taps, not collinear, or there is no fit
};
// support: the counting taps per pixel, where it is asked for.  Throws std::runtime_error where pm_disparity_normals refuses.
core::Image<core::Vec3f> DisparityNormals(const core::Image<float>& disp, const StereoModel& model,
                                          const NormalsFit& fit = NormalsFit(), core::Image<uint8_t>* support = nullptr);
// Between Match() and the stages above: the map with every connected region of similar disparity of at most max_size
// pixels set to 0 (pm/imaging.h: pm_filter_speckles; definition: tests/speckle_ref.py).  4-neighbours are joined iff both
// are > 0 and differ by at most max_diff; nothing is filled or smoothed.
struct SpeckleFilter {  // pm_speckle_filter
  float max_diff = 1.f;  // finite, >= 0
  int max_size = 100;    // >= 0; 0 removes nothing
};
// labels: the smallest index y * cols + x of each pixel's component in the INPUT map (-1 where it is not > 0); removed: the
// number of pixels set to 0; each where it is asked for.  Throws std::runtime_error where pm_filter_speckles refuses.
core::Image<float> FilterSpeckles(const core::Image<float>& disp, const SpeckleFilter& filter = SpeckleFilter(),
                                  core::Image<int32_t>* labels = nullptr, int* removed = nullptr);
// Behind the cloud: the organised grid mesh of a map (pm/imaging.h: pm_grid_mesh; definition: tests/mesh_ref.py).  Every
// 2x2 cell of the stride grid becomes up to two triangles facing the camera, unless two of its corners differ by more than
// max_diff or do not count.
struct MeshOptions {  // pm_mesh_options
  float max_diff = 1.f;            // finite, >= 0: the largest disparity step a triangle's edge may span
  bool referenced_vertices = true; // true: only vertices some triangle names; false: every counted pixel (MakePointCloud's)
};
struct TriangleMesh {
  PointCloud vertices;
  std::vector<std::array<int32_t, 3>> triangles;  // indices into `vertices`, in row-major cell order
};
// Counts first, then sizes the buffers exactly.  Throws std::runtime_error where pm_grid_mesh refuses.
TriangleMesh MakeGridMesh(const core::Image<float>& disp, const StereoModel& model, const CloudFilter& filter = CloudFilter(),
                          const MeshOptions& options = MeshOptions(), const core::Image<core::Vec3f>* normals = nullptr,
                          const core::Image<core::Vec3b>* bgr = nullptr);
// Host only: the mesh as a binary little-endian PLY file -- element vertex with float x y z, float nx ny nz where the mesh
// has normals and uchar red green blue where it has colour; element face with `list uchar int vertex_indices`.  Throws
// std::runtime_error where the file cannot be written.
void WritePly(const std::string& path, const TriangleMesh& mesh);

// Between two frames of a sequence: the OLD frame's left map carried into the NEW frame's two seed maps through the rigid
// motion between the two left cameras (pm/imaging.h: pm_reproject_disparity; definition: tests/reproject_ref.py).  Unlike
// the functions above it takes DEVICE pointers and works on the matcher's own handle and stream, because that is where a
// sequence lives: the maps a device Match() left behind go in, and the seeds go to pm_submit_device_after behind an event
// recorded on pm_stream(matcher.handle()).
struct Motion {  // pm_motion: X_new = R X_old + t between the left camera frames, R row-major
  std::array<double, 9> R{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
  std::array<double, 3> t{{0, 0, 0}};
};
struct ReprojectOptions {  // pm_reproject_options
  float min_disp = 0.f;  // a source pixel takes part iff disp > 0 and disp >= min_disp
  float max_disp = 0.f;  // > 0: a carried disparity above it is dropped; 0 = no limit
  int close_radius = 1;  // 0..3: holes take the maximum of their (2 r + 1)^2 window
};
// Host only: T_new_old = T_world_new^-1 * T_world_old for two rigid 4x4 poses of the left camera (camera to world,
// row-major; the last row is taken to be 0 0 0 1 and the rotation block to be orthonormal).
Motion RelativeMotion(const double T_world_old[16], const double T_world_new[16]);
// d_seed_l / d_seed_r: device maps of rows x cols floats, either may be null.  Returns {pixels > 0 of d_seed_l, of d_seed_r}
// and synchronises the matcher's stream for them; with want_counts = false it only enqueues and returns {-1, -1}.  The
// matcher must have planned its handle (Params::max_rows / max_cols, or a first Match()).  Throws std::runtime_error where
// pm_reproject_disparity refuses.
std::array<int, 2> ReprojectDisparity(pm::PatchmatchGpu& matcher, const StereoModel& model, const Motion& motion,
                                      const float* d_disp, int rows, int cols, float* d_seed_l, float* d_seed_r,
                                      const ReprojectOptions& options = ReprojectOptions(), bool want_counts = true);

// Along a sequence: the CURRENT left map judged by earlier left maps of the same size and camera, each reached through the
// motion X_src = R X_cur + t between the left camera frames -- RelativeMotion(T_world_cur, T_world_src) (pm/imaging.h:
// pm_filter_consistency; definition: tests/consistency_ref.py).  A pixel > 0 is kept iff at least min_consistent sources saw
// the same surface (within max_diff, nearest of a (2 radius + 1)^2 window) and at most max_conflicts saw through it.
struct ConsistencyOptions {  // pm_consistency_options
  float max_diff = 1.f;    // finite, >= 0
  int radius = 1;          // 0..2
  int min_consistent = 1;  // 0..sources.size()
  int max_conflicts = 0;   // 0..8
};
// Host images in, host images out, on the matcher's own handle and stream (pm_device_malloc / pm_upload / pm_download):
// out: disp with every pixel > 0 that is not kept set to 0; classes: the class of source k (0 unseen, 1 consistent,
// 2 occluded, 3 conflict) in bits 2k, 2k + 1; residual: the mean |difference| over the consistent sources; each where it
// is asked for.  Returns {pixels > 0, kept pixels}.  The matcher must have planned its handle.  Throws
// std::invalid_argument where the sizes differ and std::runtime_error where pm_filter_consistency refuses.
std::array<int, 2> FilterConsistency(pm::PatchmatchGpu& matcher, const StereoModel& model,
                                     const std::vector<core::Image<float>>& sources, const std::vector<Motion>& motions,
                                     const ConsistencyOptions& options, const core::Image<float>& disp,
                                     core::Image<float>* out, core::Image<uint16_t>* classes = nullptr,
                                     core::Image<float>* residual = nullptr);

// Matching confidence of a left disparity map over its rectified 8-bit pair (pm/imaging.h: pm_disparity_confidence;
// definition: tests/confidence_ref.py).  The matching functor of the matcher's handle is evaluated again at d, at d - 1 and
// d + 1 and at the background hypothesis 0 over a patch_w x patch_h window; with disp_r the left-right residual is read too.
// A measured pixel (d > 0, the window inside the image, d <= x - patch_w / 2) is kept iff it passes every threshold.
struct ConfidenceOptions {  // pm_confidence_options
  int patch_w = 7, patch_h = 7;                 // odd, 3 .. PM_MAX_PATCH
  float max_cost = HUGE_VALF;                   // cost(d) <= max_cost
  float min_margin = -HUGE_VALF;                // min(cost(d - 1), cost(d + 1)) - cost(d) >= min_margin
  float min_bg_margin = -HUGE_VALF;             // cost(0) - cost(d) >= min_bg_margin
  float max_lr_diff = HUGE_VALF;                // |disp_r(y, x - d) - d| <= max_lr_diff, read only with disp_r
  bool drop_unmeasured = false;                 // also zero the pixels > 0 that are not measured
};
struct ConfidenceMeasures {  // the four planes of d_measures; a pixel that is not measured holds -1, 0, 0, +inf
  core::Image<float> cost, margin, bg_margin, lr;
};
// out: the map with the measured pixels that fail zeroed (may be &disp_l); measures: the four measures; flags: PM_CONF_* bits
// per pixel; each where it is asked for.  disp_r may be null.  Returns {pixels > 0, measured pixels, kept pixels}.  The matcher
// must have planned its handle.  Throws std::invalid_argument where the sizes differ or an image is not packed and
// std::runtime_error where pm_disparity_confidence refuses.
std::array<int, 3> DisparityConfidence(pm::PatchmatchGpu& matcher, const core::Image<uint8_t>& left,
                                       const core::Image<uint8_t>& right, const ConfidenceOptions& options,
                                       const core::Image<float>& disp_l, const core::Image<float>* disp_r,
                                       core::Image<float>* out, ConfidenceMeasures* measures = nullptr,
                                       core::Image<uint8_t>* flags = nullptr);

// Along a sequence: the CURRENT left map refined by, and filled from, earlier left maps of the same size and camera, each
// reached through the motion X_src = R X_cur + t -- RelativeMotion(T_world_cur, T_world_src) (pm/imaging.h:
// pm_fuse_disparity; definition: tests/fuse_ref.py).  A kept pixel > 0 becomes the weighted mean of itself and of what the
// consistent sources observed along its ray; with fill_min_sources >= 1 a pixel without a value takes the mean of the sources
// that agree, within fill_max_diff, with the nearest surface they carry to it.
struct FuseOptions {  // pm_fuse_options
  float max_diff = 1.f;      // finite, >= 0
  int radius = 1;            // 0..2
  int min_consistent = 1;    // 0..sources.size()
  int max_conflicts = 0;     // 0..8
  int fill_min_sources = 0;  // 0: no fill; else 1..sources.size()
  float fill_max_diff = 1.f;  // finite, >= 0
};
// Host images in, host images out, on the matcher's own handle and stream.  weight: the current map's weight plane, may be
// null; source_weights: empty, or one entry per source, an empty image standing for "no plane" (1.0 everywhere).  out: the
// fused map; count: the observations per pixel; spread: their range; flags: PM_FUSE_* bits; each where it is asked for.
// Returns {pixels > 0, kept, fused, filled}.  The matcher must have planned its handle.  Throws std::invalid_argument where
// the sizes differ and std::runtime_error where pm_fuse_disparity refuses.
std::array<int, 4> FuseDisparity(pm::PatchmatchGpu& matcher, const StereoModel& model,
                                 const std::vector<core::Image<float>>& sources, const std::vector<Motion>& motions,
                                 const FuseOptions& options, const core::Image<float>& disp, const core::Image<float>* weight,
                                 const std::vector<core::Image<float>>& source_weights, core::Image<float>* out,
                                 core::Image<uint8_t>* count = nullptr, core::Image<float>* spread = nullptr,
                                 core::Image<uint8_t>* flags = nullptr);

// The motion of the left camera between two frames, X_new = R X_old + t: what ReprojectDisparity takes, and, the other way
// round, what FilterConsistency and FuseDisparity take (pm/imaging.h: pm_track_features, pm_solve_motion, pm_estimate_motion;
// definition: tests/motion_ref.py).  One corner per cell of the old left image with a value in its disparity map is predicted
// through the guess and block-matched in the new left image; the motion is fitted to the tracks on the host in binary64.
struct TrackOptions {  // pm_track_options
  int cell = 16;             // 8..64
  int patch_radius = 3;      // 1..7
  int search_radius = 5;     // 0..24
  int64_t min_score = 1;     // >= 1
  float min_disp = 0.f, max_disp = 0.f;  // >= 0; max_disp 0 = no limit
  int max_sad = 0;           // >= 0, 0 = no limit
  int min_gap = 0;           // >= 0
};
struct SolveOptions {  // pm_solve_options
  int iterations = 10;      // 1..50
  double huber_px = 1.0;    // > 0
  double epsilon = 1e-9;    // >= 0
  double inlier_px = 1.0;   // > 0
  int min_inliers = 12;     // >= 6
};
// Host images in, the records out (all of them), on the matcher's own handle and stream; guess: null = the identity.  The
// matcher must have planned its handle.  Throws std::invalid_argument where the sizes differ and std::runtime_error where
// pm_track_features refuses.
std::vector<pm_track> TrackFeatures(pm::PatchmatchGpu& matcher, const StereoModel& model, const TrackOptions& options,
                                    const Motion* guess, const core::Image<uint8_t>& left_old, const core::Image<float>& disp_old,
                                    const core::Image<uint8_t>& left_new);
// No device takes part.  info->valid == 0: the result is not to be trusted and the returned motion is the guess.  Throws
// std::runtime_error where pm_solve_motion refuses.
Motion SolveMotion(const StereoModel& model, const SolveOptions& options, const std::vector<pm_track>& tracks, const Motion* guess,
                   pm_motion_info* info = nullptr);
// TrackFeatures, then SolveMotion, in one call of the C ABI (pm_estimate_motion).
Motion EstimateMotion(pm::PatchmatchGpu& matcher, const StereoModel& model, const TrackOptions& track_options,
                      const SolveOptions& solve_options, const Motion* guess, const core::Image<uint8_t>& left_old,
                      const core::Image<float>& disp_old, const core::Image<uint8_t>& left_new, pm_motion_info* info = nullptr);

// Dense alignment of a NEW left disparity map against a MODEL's map and camera-facing normals (TsdfVolume::Raycast's outputs,
// or an earlier map with DisparityNormals / PlaneNormals): point-to-plane Gauss-Newton with projective association
// (pm/imaging.h: pm_align_disparity; definition: tests/align_ref.py).  The motion goes from the model camera's frame into the new
// camera's, X_new = R X_model + t: what ReprojectDisparity takes.  info->valid == 0: the result is not to be trusted and the
// returned motion is the guess.  Runs on the matcher's handle; throws std::runtime_error where the C call refuses.
struct AlignOptions {  // pm_align_options
  float min_disp = 0.f;    // a pixel takes part iff disp > 0 and disp >= min_disp
  float max_diff = 1.f;    // the gate between the carried and the measured disparity, pixels; finite, >= 0
  double huber_px = 1.0;   // > 0
  int iterations = 10;     // 1..50
  double epsilon = 1e-9;   // >= 0: stop when no entry of the update exceeds it
  int min_used = 100;      // >= 6
};
Motion AlignDisparity(pm::PatchmatchGpu& matcher, const StereoModel& model, const AlignOptions& options, const Motion* guess,
                      const core::Image<float>& disp_model, const core::Image<core::Vec3f>& normals_model,
                      const core::Image<float>& disp_new, pm_align_info* info = nullptr);
// AlignDisparity with a PHOTOMETRIC term blended in: the model's colour (TsdfVolume::ColorMap at the render's pose; zeros = not
// coloured) against the new frame's image, bytes or floats (pm/imaging.h: pm_align_color_disparity; definition:
// tests/align_photo_ref.py).  It constrains what point-to-plane leaves free on a flat scene.  info->geo.valid == 0: the returned
// motion is the guess.
struct AlignColorOptions {  // pm_align_color_options
  AlignOptions align;          // the geometric term and the loop
  double huber_levels = 20.0;  // > 0: the Huber threshold of the photometric residual, in levels
  double lambda = 0.03;        // finite, >= 0: levels into pixels of disparity (sigma_d / sigma_I)
};
Motion AlignColorDisparity(pm::PatchmatchGpu& matcher, const StereoModel& model, const AlignColorOptions& options,
                           const Motion* guess, const core::Image<float>& disp_model, const core::Image<core::Vec3f>& normals_model,
                           const core::Image<core::Vec3f>& bgr_model, const core::Image<float>& disp_new,
                           const core::Image<core::Vec3b>& bgr_new, pm_align_color_info* info = nullptr);
Motion AlignColorDisparity(pm::PatchmatchGpu& matcher, const StereoModel& model, const AlignColorOptions& options,
                           const Motion* guess, const core::Image<float>& disp_model, const core::Image<core::Vec3f>& normals_model,
                           const core::Image<core::Vec3f>& bgr_model, const core::Image<float>& disp_new,
                           const core::Image<core::Vec3f>& bgr_new, pm_align_color_info* info = nullptr);
// Host only: X -> a(b(X)) (pm_motion_compose).  The pose of a frame aligned against a render at pose_ref is
// ComposeMotion(M, pose_ref).
Motion ComposeMotion(const Motion& a, const Motion& b);

// A persistent world-frame model of a sequence: a truncated signed distance volume that Integrate folds left disparity maps
// and their camera poses into and Raycast renders back, at any pose, as an ordinary left disparity map with normals -- what
// MakePointCloud, MakeGridMesh, ReprojectDisparity (with the identity motion, for the right seed), FilterConsistency and
// FuseDisparity take (pm/imaging.h: pm_tsdf_clear, pm_tsdf_integrate, pm_tsdf_raycast; definition: tests/tsdf_ref.py) -- and that Mesh takes out
// whole, as one triangle mesh in the world frame (pm_tsdf_mesh).  A pose is
// a Motion from the WORLD frame into the left camera's: X_cam = R X_world + t.
struct TsdfGrid {  // pm_tsdf_volume
  int nx = 0, ny = 0, nz = 0;               // voxels, x fastest
  std::array<double, 3> origin{{0, 0, 0}};  // the world position of the centre of voxel (0, 0, 0)
  double voxel = 0.01;                      // edge length, > 0
  double trunc = 0.04;                      // truncation distance, > 0 (typically 3..5 voxels)
  float max_weight = 64.f;                  // > 0: the weight saturates here
};
struct TsdfIntegrateOptions {  // pm_tsdf_integrate_options
  float min_disp = 0.f;   // a pixel measures iff disp > 0 and disp >= min_disp
  float max_range = 0.f;  // > 0: a measured range above it is dropped; 0 = no limit
};
struct TsdfMeshOptions {  // pm_tsdf_mesh_options
  float min_weight = 0.f;  // a node is observed iff weight > 0, weight >= min_weight and its value is finite
};
struct TsdfColorOptions {  // pm_tsdf_color_options
  float min_disp = 0.f;   // TsdfIntegrateOptions' two
  float max_range = 0.f;
  float band = 1.f;       // in (0, 1]: a voxel takes the pixel's colour iff |sdf| <= band * trunc
};
struct TsdfColorSampleOptions {  // pm_tsdf_color_sample_options
  float min_weight = 0.f;  // a corner takes part iff its colour weight is > 0 and >= min_weight
  float byte_scale = 1.f;  // finite, > 0: bytes = saturate(rint(value * byte_scale)); 255 for float images in [0, 1]
};
struct TsdfRaycastOptions {  // pm_tsdf_raycast_options
  float min_range = 0.1f, max_range = 10.f;  // finite, 0 < min_range < max_range
  float step = 0.5f;                         // the march's step as a fraction of trunc, in (0, 1]
  float min_weight = 0.f;                    // a voxel takes part iff weight > 0 and weight >= min_weight
};
// Owns the volume's device memory (8 bytes per voxel, 8 + 16 with a colour volume) on the matcher's handle, which must be
// planned and must outlive the volume; everything runs on that handle's stream.  Throws std::invalid_argument for a grid
// pm_tsdf_bytes refuses and where image sizes differ, std::runtime_error where the C call refuses.
// With with_color it owns a colour volume too (16 bytes per voxel: b, g, r, weight; pm/imaging.h: pm_tsdf_color_*; definition:
// tests/tsdf_color_ref.py), which IntegrateColor fuses the frames' images into and ColorMap, ColorPoints and Mesh(want_color) read
// back; without it those throw std::logic_error.
class TsdfVolume {
 public:
  TsdfVolume(pm::PatchmatchGpu& matcher, const TsdfGrid& grid, bool with_color = false);  // allocated and cleared
  ~TsdfVolume();
  TsdfVolume(const TsdfVolume&) = delete;
  TsdfVolume& operator=(const TsdfVolume&) = delete;
  const TsdfGrid& grid() const { return grid_; }
  size_t voxels() const { return (size_t)grid_.nx * grid_.ny * grid_.nz; }
  void* device();  // nx * ny * nz records {float tsdf; float weight}
  bool has_color() const;
  void* color_device();  // nx * ny * nz records {float b, g, r, weight}; null without a colour volume
  void Clear();          // both volumes
  // Host map in; weight: a plane of the map's size, null = 1.0.  Returns {voxels in view, voxels updated}.
  std::array<int, 2> Integrate(const StereoModel& model, const Motion& pose, const core::Image<float>& disp,
                               const core::Image<float>* weight = nullptr,
                               const TsdfIntegrateOptions& options = TsdfIntegrateOptions());
  // Device maps in (those a device Match() left behind); with want_counts = false it only enqueues and returns {-1, -1}.
  std::array<int, 2> IntegrateDevice(const StereoModel& model, const Motion& pose, const float* d_disp, const float* d_weight,
                                     int rows, int cols, const TsdfIntegrateOptions& options = TsdfIntegrateOptions(),
                                     bool want_counts = true);
  // Integrate, and the image the map came with -- bytes or floats, the map's size -- fused into the colour volume.  Returns
  // {voxels in view, updated, coloured}.
  std::array<int, 3> IntegrateColor(const StereoModel& model, const Motion& pose, const core::Image<float>& disp,
                                    const core::Image<core::Vec3b>& bgr, const core::Image<float>* weight = nullptr,
                                    const TsdfColorOptions& options = TsdfColorOptions());
  std::array<int, 3> IntegrateColor(const StereoModel& model, const Motion& pose, const core::Image<float>& disp,
                                    const core::Image<core::Vec3f>& bgr, const core::Image<float>* weight = nullptr,
                                    const TsdfColorOptions& options = TsdfColorOptions());
  // Device buffers in, exactly one of d_bgr8 and d_bgr; with want_counts = false it only enqueues and returns {-1, -1, -1}.
  std::array<int, 3> IntegrateColorDevice(const StereoModel& model, const Motion& pose, const float* d_disp, const float* d_weight,
                                          const uint8_t* d_bgr8, const float* d_bgr, int rows, int cols,
                                          const TsdfColorOptions& options = TsdfColorOptions(), bool want_counts = true);
  // The fused colour at the pixels of any left map at `pose` -- a Raycast of the model, or a measured map: floats and bytes, each
  // where it is asked for (at least one); zeros where a pixel has no value or no colour.  Returns the pixels coloured.
  int ColorMap(const StereoModel& model, const Motion& pose, const core::Image<float>& disp, core::Image<core::Vec3f>* bgr,
               core::Image<core::Vec3b>* bgr8 = nullptr, const TsdfColorSampleOptions& options = TsdfColorSampleOptions());
  int ColorMapDevice(const StereoModel& model, const Motion& pose, const float* d_disp, int rows, int cols, float* d_bgr_out,
                     uint8_t* d_bgr8_out, const TsdfColorSampleOptions& options = TsdfColorSampleOptions(), bool want_counts = true);
  // The fused colour at world-frame points; each output where it is asked for (at least one).  Returns the points coloured.
  int ColorPoints(const std::vector<core::Vec3f>& xyz, std::vector<core::Vec3f>* bgr, std::vector<core::Vec3b>* bgr8 = nullptr,
                  const TsdfColorSampleOptions& options = TsdfColorSampleOptions());
  // Host images out, each where it is asked for (at least one).  Returns the pixels hit.
  int Raycast(const StereoModel& model, const Motion& pose, int rows, int cols, core::Image<float>* disp,
              core::Image<core::Vec3f>* normals = nullptr, const TsdfRaycastOptions& options = TsdfRaycastOptions());
  // Device maps out: d_disp_out rows x cols floats, d_normals_out rows x cols x 3 floats, either may be null; with
  // want_counts = false it only enqueues and returns -1.
  int RaycastDevice(const StereoModel& model, const Motion& pose, int rows, int cols, float* d_disp_out, float* d_normals_out,
                    const TsdfRaycastOptions& options = TsdfRaycastOptions(), bool want_counts = true);
  // The model taken out of the volume: its zero level set as ONE welded triangle mesh in the WORLD frame, one vertex per
  // crossed grid edge (pm/imaging.h: pm_tsdf_mesh; definition: tests/tsdf_mesh_ref.py).  A count call, then one call sized to
  // fit.  vertices.xyz always, vertices.normals (toward free space; (0, 0, 0) where the volume's gradient is not known) with
  // want_normals; vertices.bgr (the fused colour through pm_tsdf_color_points, on the device behind pm_tsdf_mesh; (0, 0, 0) where
  // a vertex has none) with want_color; no index.  WritePly takes the result unchanged, colour included.
  TriangleMesh Mesh(const TsdfMeshOptions& options = TsdfMeshOptions(), bool want_normals = true, bool want_color = false,
                    const TsdfColorSampleOptions& color_options = TsdfColorSampleOptions());
  // Device streams out, each may be null: d_xyz_out and d_normals_out vertex_capacity x 3 floats, d_tri_out tri_capacity x 3
  // int32, d_counts two device ints.  Returns {vertices, triangles}, both counted beyond the capacities; with want_counts =
  // false it only enqueues and returns {-1, -1}.
  std::array<int, 2> MeshDevice(const TsdfMeshOptions& options, int vertex_capacity, int tri_capacity, float* d_xyz_out,
                                float* d_normals_out, int32_t* d_tri_out, int* d_counts = nullptr, bool want_counts = true);
  // Tracking against the model: raycasts at pose_guess into device buffers the volume owns, aligns disp_new against that render
  // from the identity (AlignDisparity) and returns ComposeMotion(M, pose_guess), the new frame's pose; pose_guess itself where
  // info->valid == 0.
  Motion Align(const StereoModel& model, const Motion& pose_guess, const core::Image<float>& disp_new,
               const TsdfRaycastOptions& raycast_options = TsdfRaycastOptions(), const AlignOptions& align_options = AlignOptions(),
               pm_align_info* info = nullptr);
  // Align with colour, for a volume that has a colour volume: raycast and ColorMapDevice at pose_guess, AlignColorDisparity's loop
  // from the identity against that render, ComposeMotion(M, pose_guess); pose_guess itself where info->geo.valid == 0.
  Motion AlignColor(const StereoModel& model, const Motion& pose_guess, const core::Image<float>& disp_new,
                    const core::Image<core::Vec3b>& bgr_new, const TsdfRaycastOptions& raycast_options = TsdfRaycastOptions(),
                    const AlignColorOptions& align_options = AlignColorOptions(),
                    const TsdfColorSampleOptions& color_options = TsdfColorSampleOptions(), pm_align_color_info* info = nullptr);
  Motion AlignColor(const StereoModel& model, const Motion& pose_guess, const core::Image<float>& disp_new,
                    const core::Image<core::Vec3f>& bgr_new, const TsdfRaycastOptions& raycast_options = TsdfRaycastOptions(),
                    const AlignColorOptions& align_options = AlignColorOptions(),
                    const TsdfColorSampleOptions& color_options = TsdfColorSampleOptions(), pm_align_color_info* info = nullptr);
  // The records, 2 floats per voxel (tsdf, weight), x fastest; synchronises.
  std::vector<float> Download();

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
  TsdfGrid grid_;
};

}  // namespace imaging
}  // namespace bm
