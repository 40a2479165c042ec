/* pm/imaging.h -- C ABI of the range-dependent post-processing that follows the stereo hot path
 * (SURVEY.md section 8, row f-3): disparity -> range -> Sea-thru style correction, per pixel.
 *
 * Replaces, for device-resident images:
 *   - StereoCamera::DispToDepth            src/vehicle/vision_core/stereo_camera.cpp:49-53
 *   - imaging::RemoveBackscatter           src/vehicle/imaging/backscatter.cpp:277-308
 *   - imaging::CorrectAttenuation          src/vehicle/imaging/attenuation.cpp:269-299
 *     (with SetMaxRangeWhereZero, :255-266)
 *   - ComputeIntensity                     src/vehicle/vision_core/image_util.cpp:97-102
 *   - imaging::FindDarkFast                src/vehicle/imaging/backscatter.cpp:41-78
 *   - imaging::EstimateIlluminantRangeGuided src/vehicle/imaging/illuminant.cpp:24-34
 *     (fastGuidedFilter with a one-channel guide, src/vehicle/imaging/fast_guided_filter.cpp)
 * i.e. every whole-image stage of imaging::EnhanceUnderwater (src/vehicle/imaging/enhance.cpp:22-85).
 * The Levenberg-Marquardt parameter fits (EstimateBackscatter, EstimateBeta) stay with the caller: they
 * work on <= a few hundred sampled pixels, which pm_gather_pixels fetches, and hand over B, beta_B, beta_D.
 *
 * Conventions: all image pointers are DEVICE memory, tightly packed; Image3f is interleaved BGR
 * float ([rows][cols][3]) like cv::Mat_<cv::Vec3f>; Image1f is [rows][cols] float.  Every function
 * enqueues on the handle's stream (pm_stream) and returns; pm_synchronize waits.  A disparity map
 * produced by pm_match_device on the same handle can therefore be consumed without a host round trip.
 * Arithmetic is float, in the reference's operation order; exp is the device's correctly-rounded-to-1-ulp
 * expf, so results agree with a host evaluation to a few ulp (tests state 1e-5 relative), not bit for bit.
 */
#ifndef PM_IMAGING_H_
#define PM_IMAGING_H_

#include "pm/patchmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* range = (float)(fx * baseline / (double)disp) where disp > 0, else 0 ("no range", the value
 * RemoveBackscatter / CorrectAttenuation treat as background).  DispToDepth CHECK-fails on disp <= 0;
 * its callers skip those pixels (src/vehicle/mesher/object_mesher.cpp uses only tracked features). */
int pm_disp_to_range(pm_handle* h, const float* d_disp, int rows, int cols, double fx, double baseline,
                     float* d_range);

/* out = max(bgr - B * (1 - exp(-beta_B * z)), 0) per channel, z = range where range > 1e-3 else
 * range + 20 m (kBackgroundRange, backscatter.cpp:18). */
int pm_remove_backscatter(pm_handle* h, const float* d_bgr, const float* d_range, int rows, int cols,
                          const float B[3], const float beta_B[3], float* d_out);

/* out = bgr * exp(z * (a * exp(b z) + c * exp(d z))) per channel, X = (a_bgr, b_bgr, c_bgr, d_bgr),
 * z = range where range > 0 else range + max(range) (SetMaxRangeWhereZero). */
int pm_correct_attenuation(pm_handle* h, const float* d_bgr, const float* d_range, int rows, int cols,
                           const float X[12], float* d_out);

/* The three in one pass over the image: disparity map in, corrected image out (and the range map if
 * d_range_out is not NULL).  Equals pm_disp_to_range -> pm_remove_backscatter -> pm_correct_attenuation. */
int pm_range_enhance(pm_handle* h, const float* d_bgr, const float* d_disp, int rows, int cols, double fx,
                     double baseline, const float B[3], const float beta_B[3], const float X[12],
                     float* d_range_out, float* d_out);

/* gray = 0.114 B + 0.587 G + 0.299 R (cv::cvtColor BGR2GRAY on floats). */
int pm_compute_intensity(pm_handle* h, const float* d_bgr, int rows, int cols, float* d_gray);

/* FindDarkFast: the intensity threshold under which `percentile` of the pixels with range > 0.1 lie,
 * found by the reference's 1 + 8 counting steps; writes the mask (255 / 0) of the last step tested and
 * returns the threshold through *threshold.  Synchronises the stream (the counts steer the search). */
int pm_find_dark(pm_handle* h, const float* d_intensity, const float* d_range, int rows, int cols,
                 float percentile, uint8_t* d_mask, float* threshold);

/* ---- the range-guided illuminant (EnhanceUnderwater's step between RemoveBackscatter and CorrectAttenuation) -----
 * Unlike the exp-based stages above these are held to their CPU definition (tests/guided_ref.py) BIT FOR BIT: every
 * operation is one binary32 rounding in the reference's order; the box means accumulate in binary64 like cv::blur on
 * float images, in a fixed order (the k taps of a row left to right, then the k row sums top to bottom).  Scratch for
 * the coarse image (rows / s x cols / s) is allocated on first use and reused.
 *
 * fastGuidedFilter(I = guide, p = src, r, eps, s) of fast_guided_filter.cpp:207-233 with a ONE-channel float guide
 * (FastGuidedFilterMono, :90-123); src has 1..4 interleaved float channels, each filtered on its own (:74-84).
 * dst may equal src.  scale multiplies the result (1.0f = the filter itself).  rows / s >= 1, cols / s >= 1, s >= 1,
 * r >= 0, eps finite and >= 0.  The three-channel (colour) guide of FastGuidedFilterColor (:126-204) is NOT provided:
 * nothing in the reference calls it. */
int pm_fast_guided_filter(pm_handle* h, const float* d_guide, const float* d_src, int rows, int cols, int channels,
                          int r, double eps, int s, float scale, float* d_dst);

/* EstimateIlluminantRangeGuided (illuminant.cpp:24-34): 2.0f * fastGuidedFilter(range, bgr, r, eps, s). */
int pm_estimate_illuminant_range_guided(pm_handle* h, const float* d_bgr, const float* d_range, int rows, int cols,
                                        int r, double eps, int s, float* d_illuminant);

/* n pixels (x, y) of a device image with 1..4 float channels -> host_out[n][channels]: the samples the caller's
 * fits read (EstimateBeta: range and illuminant at <= num_px grid points, attenuation.cpp:43-69), without the image
 * crossing to the host.  d_xy is a device array of n (x, y) pairs, or xy a host array (exactly one of them non-NULL).
 * A coordinate outside the image is PM_ERR_INVALID_ARG (nothing is clamped; host_out is left untouched).  Returns
 * after the values have arrived (synchronises the stream). */
int pm_gather_pixels(pm_handle* h, const float* d_img, int rows, int cols, int channels, const int32_t* d_xy,
                     const int32_t* xy, int n, float* host_out);

/* ---- range-free enhancement in FRONT of stereo ---------------------------
 * The "stereo-ready" chain of test/imaging/enhance_test.cpp:69-73 and test/stereo_matching/sgbm_test.cpp:66-84:
 *   J    = Normalize(NormalizeColorIlluminant(CastImage3bTo3f(bgr8)))
 *          (src/vehicle/imaging/normalization.cpp:43-69, :178-185; illuminant.cpp:10-21; image_util.cpp:25-31;
 *          as written there: NormalizeColorIlluminant ends with a Normalize of its own, so the value channel is
 *          stretched twice)
 *   gray = cv::cvtColor(J, BGR2GRAY), converted to 8 bit (x 255, saturate_cast) -- the image Match() consumes.
 * d_bgr8: [rows][cols][3] bytes.  d_J ([rows][cols][3] float) and d_gray8 ([rows][cols] bytes) are optional
 * outputs (at least one).  rows, cols >= 8.  Scratch for the image size is allocated on first use.
 * Edge cases, all equal to the CPU definition (oracle/pm_enhance_oracle.c) bit for bit:
 *   - a gray image delivered as BGR (b == g == r, a monochrome camera): the first stretch puts the cell that defined its
 *     minimum at 0 -+ rounding, so the second stretch's minimum may be slightly negative or -0.0; the min / max
 *     reductions order floats of either sign.
 *   - black regions: a zero illuminant divides to 0 (cv::divide), the first minimum is then exactly 0.
 *   - a CONSTANT image (all-black included): vmax == vmin, the reference's arithmetic divides by zero.  Every value of
 *     J is NaN (the second stretch sees no ordered value and keeps its initial minimum FLT_MAX and maximum -FLT_MAX) and
 *     every byte of the gray image is 0 (NaN saturates to 0).  Nothing is detected or reported: as in the reference,
 *     the caller is expected not to feed featureless frames. */
int pm_stereo_ready(pm_handle* h, const uint8_t* d_bgr8, int rows, int cols, float* d_J, uint8_t* d_gray8);

/* Match() on 8-bit BGR pairs with that enhancement FOLDED INTO THE LOAD PATH (BASELINE config 5: "underwater enhancement
 * fused into the cost kernel"): per image the two Gaussian passes of the illuminant estimate and two small min / max
 * passes run as kernels; the whole per-pixel tail -- I / (2 blur), both HSV value stretches, gray, 8 bit -- is computed
 * inside the prep kernel that produces the matcher's image / gradient planes, so neither the quotient image, nor the
 * stretched images, nor the gray image is ever written to memory.  The result equals pm_stereo_ready on both images
 * followed by pm_match_device, bit for bit, in every mode of the handle (scalar and PM_MODE_PLANES, f32 / f16 state).
 * d_left_bgr8 / d_right_bgr8: [n][rows][cols][3] bytes on the device; the other arguments as pm_match_device. */
int pm_match_bgr_device(pm_handle* h, int n, const uint8_t* d_left_bgr8, const uint8_t* d_right_bgr8, int rows, int cols,
                        const float* d_seed_l, const float* d_seed_r, float* d_disp_l, float* d_disp_r);

/* The two building blocks on float images, for callers that run them separately:
 * cv::GaussianBlur(src, dst, Size(ksize, ksize), sigma, sigma, BORDER_REPLICATE) for 1-4 interleaved channels
 * (EstimateIlluminantGaussian = 2 x this, illuminant.cpp:10-21), and imaging::Normalize. */
int pm_gaussian_blur(pm_handle* h, const float* d_src, int rows, int cols, int channels, int ksize, double sigma,
                     float* d_dst);
/* pm_normalize takes ANY float image, negative channels and all-negative pixels included (its own output has them): the
 * value channel is the largest of the three channels whatever its sign, and its minimum / maximum over the 1/8 image are
 * taken over floats of either sign, like the CPU definition, bit for bit.  NaN cells of the 1/8 image are skipped; a
 * constant image (vmax == vmin) gives NaN everywhere (see pm_stereo_ready).  rows, cols >= 8.
 * pm_gaussian_blur: ksize odd and >= 1 (1 copies the image: the single tap is 1.0f), sigma > 0; ksize may exceed the image. */
int pm_normalize(pm_handle* h, const float* d_bgr, int rows, int cols, float* d_out);
/* imaging::NormalizeColorIlluminant on a float image (normalization.cpp:178-185). */
int pm_normalize_color_illuminant(pm_handle* h, const float* d_bgr, int rows, int cols, float* d_out);

/* ---- undistortion + rectification of raw frames in FRONT of Match() ---------------------------------------------
 * Every kernel of the matcher assumes a rectified pair (pm/patchmatch.h: "rectified stereo only looks along rows").  The
 * reference ships a calibration with non-zero distortion (config/shared/ACFR.yaml:27,48) and only warns
 * "distortion_coefficients are nonzero, but we don't handle undistortion yet" (src/vehicle/params/yaml_parser.cpp:153);
 * this is the stage it lacks, as a per-frame device kernel, so that ingest -> enhancement -> Match -> range -> correction
 * never needs an image on the host.
 *
 * Like the guided filter the kernel is held to its CPU definition (tests/rectify_ref.py) BIT FOR BIT.  It is THIS
 * PROJECT'S definition: OpenCV's 15-bit coefficient table is not reproduced and nothing here claims parity with
 * cv::remap.  For destination pixel (u, v), in binary64 with one rounding per operation, parentheses as written:
 *   a = (u - cx_new) / fx_new      b = (v - cy_new) / fy_new
 *   X = (R[0] a + R[3] b) + R[6]   Y = (R[1] a + R[4] b) + R[7]   W = (R[2] a + R[5] b) + R[8]      (R^T (a, b, 1))
 *   not (W > 0): INVALID;  x = X / W, y = Y / W, xx = x x, yy = y y, xy = x y, r2 = xx + yy
 *   rad = 1 + r2 (k1 + r2 (k2 + r2 k3))
 *   tx = ((2 p1) xy) + (p2 (r2 + (2 xx)))      ty = (p1 (r2 + (2 yy))) + ((2 p2) xy)
 *   sx = fx ((x rad) + tx) + cx                sy = fy ((y rad) + ty) + cy
 *   qx = 32 sx, qy = 32 sy;  not (|qx| < 2^30 and |qy| < 2^30): INVALID (also NaN / inf)
 *   ix = rint(qx), iy = rint(qy) (half to even);  x0 = ix >> 5, ax = ix & 31, likewise y0, ay
 *   out = ((32-ax)(32-ay) p(x0,y0) + ax (32-ay) p(x0+1,y0) + (32-ax) ay p(x0,y0+1) + ax ay p(x0+1,y0+1) + 512) >> 10,
 *   a tap outside the source reads border_value; valid = 255 iff every tap with a non-zero weight lies inside, else 0.
 *   INVALID: out = border_value, valid = 0, map entry (INT32_MIN, INT32_MIN).
 * No coordinate map is kept in memory: the view travels in the kernel arguments and the model is evaluated per pixel
 * in registers, so a change of calibration allocates and invalidates nothing. */
typedef struct pm_camera { double fx, fy, cx, cy, k1, k2, p1, p2, k3; } pm_camera; /* radial-tangential model */
/* cam: the raw camera; R (3x3, row-major) rotates raw-camera coordinates into rectified ones, x_rect = R x_raw; the new
 * pinhole of the rectified image. */
typedef struct pm_rectify_view { pm_camera cam; double R[9]; double fx_new, fy_new, cx_new, cy_new; } pm_rectify_view;

/* n raw images [n][src_rows] rows of src_step bytes (0 = packed) -> n rectified images [n][rows][cols], packed.
 * d_valid ([n][rows][cols], 255 / 0) may be NULL.  stream: a hipStream_t or NULL = the handle's stream (as in
 * pm_match_view_device), so that a sequence caller can rectify on its own stream and hand the event to
 * pm_submit_device_after.
 * PM_ERR_INVALID_ARG (nothing is enqueued): a null view / d_src / d_dst, n / rows / cols / src_rows / src_cols < 1,
 * src_step smaller than src_cols, border_value outside 0 .. 255, a non-finite view entry, fx_new or fy_new == 0. */
int pm_rectify_u8(pm_handle* h, const pm_rectify_view* view, const uint8_t* d_src, int n, int src_rows, int src_cols,
                  size_t src_step, int rows, int cols, int border_value, uint8_t* d_dst, uint8_t* d_valid, void* stream);
/* the Q5 source coordinates the kernel uses: [rows][cols][2] int32 (x, y); INVALID = INT32_MIN twice.  Written by the
 * same kernel code that forms the pixels (a compile-time switch), on the handle's stream. */
int pm_rectify_map(pm_handle* h, const pm_rectify_view* view, int rows, int cols, int32_t* d_xy);
/* pm_rectify_u8 of both images into handle-owned scratch, then pm_match_device on them: same stream, same results,
 * in every mode of the handle; seeds / outputs as pm_match_device (NULL seeds + sparse_init self-seed on the
 * RECTIFIED pair).  border_value is 0.  rows x cols is the rectified size and is checked against the handle's plan like
 * pm_match_device's (PM_ERR_SIZE) before anything is enqueued.  The scratch (2 n rows cols bytes) is allocated on first
 * use, reused, and released with the handle; as for pm_match_device, a size must have run once before it is captured
 * (pm_capture_begin): growing the scratch synchronises the stream. */
int pm_match_raw_device(pm_handle* h, int n, const pm_rectify_view* left, const pm_rectify_view* right,
                        const uint8_t* d_left_raw, const uint8_t* d_right_raw, int src_rows, int src_cols,
                        size_t src_step, int rows, int cols, const float* d_seed_l, const float* d_seed_r,
                        float* d_disp_l, float* d_disp_r);
/* ---- the same for colour cameras: interleaved 8-bit BGR -------------------------------------------------------------
 * Every colour stage (pm_match_bgr_device, pm_stereo_ready, pm_range_enhance and the stages it is made of) takes an
 * interleaved BGR image that is already rectified.  The definition (tests/rectify_bgr_ref.py) is the one above, channel by
 * channel at the SAME Q5 coordinates: one border_value for the three channels, one mask per image, the same map
 * (pm_rectify_map).  The kernel evaluates the geometry once per destination pixel and shares the position, the weights and
 * the mask among the channels.  Bit for bit, like pm_rectify_u8.
 *
 * n raw images [n][src_rows] rows of src_step BYTES (0 = packed = 3 * src_cols) -> n rectified images, packed.  At least
 * one of d_dst_bgr8 and d_dst_bgr32f: the float image is (float)byte * (float)(1.0 / 255.0), one binary32 multiplication
 * (CastImage3bTo3f, image_util.cpp:25-31), the form the range-dependent stages take.  d_valid and stream as in
 * pm_rectify_u8.  PM_ERR_INVALID_ARG as for pm_rectify_u8, also for src_step smaller than 3 * src_cols and for a call
 * without an image output; nothing is enqueued then. */
int pm_rectify_bgr8(pm_handle* h, const pm_rectify_view* view, const uint8_t* d_src_bgr8, int n, int src_rows,
                    int src_cols, size_t src_step, int rows, int cols, int border_value,
                    uint8_t* d_dst_bgr8 /* [n][rows][cols][3], may be NULL */,
                    float* d_dst_bgr32f /* [n][rows][cols][3], may be NULL */,
                    uint8_t* d_valid /* [n][rows][cols], may be NULL */, void* stream);
/* pm_rectify_bgr8 of both images (border_value 0), then pm_match_bgr_device on them: same stream, same results, in every
 * mode of the handle; seeds / outputs as pm_match_bgr_device.  d_left_rect_bgr8 / d_right_rect_bgr8 ([n][rows][cols][3])
 * are optional outputs: one that is given receives the rectified image and the match reads it from there -- the left one
 * is the colour image in the geometry of the disparity map, what pm_range_enhance takes (as floats: pm_rectify_bgr8's
 * d_dst_bgr32f) -- and one that is NULL is replaced by handle-owned scratch (3 n rows cols bytes each), allocated on first
 * use, reused and released with the handle.  Size checks and the note on capture as for pm_match_raw_device. */
int pm_match_raw_bgr_device(pm_handle* h, int n, const pm_rectify_view* left, const pm_rectify_view* right,
                            const uint8_t* d_left_raw_bgr8, const uint8_t* d_right_raw_bgr8, int src_rows, int src_cols,
                            size_t src_step, int rows, int cols, const float* d_seed_l, const float* d_seed_r,
                            float* d_disp_l, float* d_disp_r, uint8_t* d_left_rect_bgr8 /* optional out */,
                            uint8_t* d_right_rect_bgr8 /* optional out */);
/* Host only, no handle, no device: rectifying rotations and a common pinhole for a calibrated pair,
 * X2 = R X1 + T (camera 1 = left).  Returns the rectified baseline (> 0) through *baseline.
 * Bouguet's construction: each camera is turned by half of R (camera 1 by R^(1/2), camera 2 by R^(-1/2)), then one
 * rotation about the axis t x (-1, 0, 0) takes the turned baseline t = R^(-1/2) T onto the -x axis, so that
 * v2->R T = (-baseline, 0, 0).  The common pinhole is fx_new = fy_new = min(c1.fy, c2.fy), (cx_new, cy_new) the mean of
 * the two principal points; there is no ROI or alpha logic.  R = I and T = (-B, 0, 0) give v1->R = v2->R = I exactly.
 * PM_ERR_INVALID_ARG: a null pointer, a non-finite entry, T = 0, a relative rotation of (nearly) 180 degrees, or a
 * turned baseline that does not point towards -x (camera 1 is not the left one). */
int pm_stereo_rectify(const pm_camera* c1, const pm_camera* c2, const double R[9], const double T[3],
                      pm_rectify_view* v1, pm_rectify_view* v2, double* baseline);

/* ---- from a disparity map to what a mapping or meshing consumer takes: points, normals, a compacted cloud ------------
 * The reference's consumers of disparity all do LeftCamera().Backproject(pixel, DispToDepth(disp))
 * (src/vehicle/mesher/object_mesher.cpp:146-150, src/vehicle/vio/stereo_frontend.cpp:119,
 * src/vehicle/vision_core/pinhole_camera.cpp:41-45) pixel by pixel on the host; these stages do it for a whole map that
 * stays on the device.  Like the guided filter and the rectification they are held to their CPU definition
 * (tests/pointcloud_ref.py) BIT FOR BIT; every operation is one rounding, parentheses as written:
 *   point   fxB = fx * baseline, formed once on the host in binary64; per pixel (x, y) with disparity d, in binary64:
 *             Zd = fxB / (double)d     Xd = (((double)x - cx) * Zd) / fx     Yd = (((double)y - cy) * Zd) / fy
 *           P = ((float)Xd, (float)Yd, (float)Zd): its Z is pm_disp_to_range's value bit for bit.
 *   normal  from the plane (a, b, z) PM_MODE_PLANES keeps per pixel, converted exactly to binary64 (f16 state included):
 *             nx = a * fx     ny = b * fy     nz = z - ((a * ((double)x - cx)) + (b * ((double)y - cy)))
 *           -- the 3-D plane through the pixel: n . P = fx * baseline > 0, so -n faces the camera -- each rounded to
 *           binary32, then in binary32  s = ((nx*nx) + (ny*ny)) + (nz*nz),  l = sqrtf(s),
 *           out = (-(nx / l), -(ny / l), -(nz / l)); (0, 0, 0) if l is not finite or not > 0.
 * All pointers are device memory, images tightly packed; every call enqueues on the handle's stream and returns a status. */
typedef struct pm_cloud_camera { double fx, fy, cx, cy, baseline; } pm_cloud_camera;
/* the rectified pinhole: pm_rectify_view's fx_new .. cy_new and pm_stereo_rectify's *baseline */

typedef struct pm_cloud_filter {
  float min_disp;   /* a pixel counts iff disp > 0 and disp >= min_disp (NaN never counts)      */
  float max_range;  /* > 0: and iff Z <= max_range (binary32, against the point's Z); 0 = no limit */
  int   stride;     /* >= 1: only pixels with x % stride == 0 and y % stride == 0 are considered */
} pm_cloud_filter;

/* PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued, for all three: a null camera, a
 * non-finite camera entry, fx or fy == 0, a null required pointer, rows or cols < 1.  PM_ERR_SIZE: more than 2^31 - 1
 * pixels (d_index_out is 32 bits wide). */

/* organised: d_xyz is [rows][cols][3] floats, (0, 0, 0) where disp is not > 0 (0, negative, NaN).  One pass, 4 bytes in
 * and 12 out per pixel. */
int pm_backproject(pm_handle* h, const pm_cloud_camera* camera, const float* d_disp, int rows, int cols, float* d_xyz);

/* organised unit normals ([rows][cols][3] floats) of the LEFT view of pair `pair`, facing the camera, read from the
 * handle's RESIDENT plane state: the state of the LAST match on this handle (pm_match_device and every entry point built
 * on it, or pm_planes_begin / _step / _write).  The next match overwrites it, so call this before matching again; work
 * already enqueued on the handle's stream is ordered in front of it.  (0, 0, 0) where the state's z is not > 0 and, if
 * d_disp_l is given, where d_disp_l is not > 0 -- pass the left map of that match to apply the cross-check's mask.
 * PM_ERR_STATE: the handle is not in PM_MODE_PLANES, or holds no state for `pair` at rows x cols; the call is valid
 * exactly when pm_planes_read is.  The scalar mode keeps no slopes: its normals come from pm_disparity_normals below. */
int pm_planes_normals(pm_handle* h, int pair, const pm_cloud_camera* camera, const float* d_disp_l /* may be NULL */,
                      int rows, int cols, float* d_normals);

/* the compacted cloud in ROW-MAJOR ORDER: the k-th counted pixel goes to slot k of every output that is given.  Points are
 * pm_backproject's, normals are copied from the organised d_normals, colour bytes from d_bgr8 (e.g. the d_left_rect_bgr8
 * of pm_match_raw_bgr_device: the colour image in the geometry of the map), d_index_out receives y * cols + x.
 * An output requires its input: d_normals_out without d_normals, or d_bgr8_out without d_bgr8, is PM_ERR_INVALID_ARG,
 * as are stride < 1, capacity < 0, a NaN min_disp and a max_range that is not >= 0.
 * *count (host) and *d_count (device) receive the number of counted pixels EVEN WHEN IT EXCEEDS capacity; then exactly
 * the first `capacity` points in row-major order are written and nothing behind them: count > capacity tells the caller
 * that the cloud was truncated.  capacity == 0 is legal and only counts (the outputs may then be NULL).  A non-NULL
 * `count` synchronises the stream like pm_find_dark; with count == NULL the call only enqueues.
 * Three small launches (per-block counts by wavefront ballot, one block of exclusive offsets, scatter); the order comes
 * from that arithmetic, never from atomics, so the result is reproducible bit for bit.  Scratch for the block offsets
 * (4 bytes per 256 considered pixels) is allocated on first use, reused, and released with the handle; growing it
 * synchronises the stream, so a size must have run once before it is captured. */
int pm_point_cloud(pm_handle* h, const pm_cloud_camera* camera, const pm_cloud_filter* filter, const float* d_disp,
                   const float* d_normals /* organised, may be NULL */,
                   const uint8_t* d_bgr8 /* [rows][cols][3], may be NULL */, int rows, int cols, int capacity,
                   float* d_xyz_out /* [capacity][3], may be NULL */, float* d_normals_out /* [capacity][3], may be NULL */,
                   uint8_t* d_bgr8_out /* [capacity][3], may be NULL */, int32_t* d_index_out /* [capacity], may be NULL */,
                   int* d_count /* device, may be NULL */, int* count /* host, may be NULL */);

/* ---- normals for a disparity map that carries no slopes: a windowed, edge-aware plane fit per pixel -------------------
 * What it is for: the d_normals input of pm_point_cloud for PM_MODE_SCALAR maps.  The scalar sweeps adopt a neighbour's
 * value, so a map is runs of equal disparities with small steps between them: finite differences are zero inside a run and
 * a spike at its edge; a least-squares plane over a (2r+1)^2 window is not.  Held to its CPU definition
 * (tests/normals_fit_ref.py) BIT FOR BIT; every operation is one rounding, parentheses and the order of the sums as written:
 *   taps    d0 = disp(y, x); not d0 > 0 (0, -0.0, negative, NaN): no fit, support 0.  A tap (dx, dy), dx, dy in -r..r,
 *           COUNTS iff (x+dx, y+dy) lies in the image, t = disp there is > 0 and fabs(e) <= (double)max_diff with
 *           e = (double)t - (double)d0 in binary64 (a NaN e never counts: d0 = +inf, the centre tap included).
 *   sums    exact integers over the counting taps: n, Sx, Sy, Sxx, Sxy, Syy of 1, dx, dy, dx^2, dx dy, dy^2; binary64,
 *           per window row dy = -r..r with dx = -r..r left to right from +0.0:  R0 = R0 + e,  R1 = R1 + ((double)dx * e);
 *           then top to bottom from +0.0:  Se = Se + R0,  Sxe = Sxe + R1,  Sye = Sye + ((double)dy * R0).
 *   solve   the integer cofactors of [[Sxx,Sxy,Sx],[Sxy,Syy,Sy],[Sx,Sy,n]]:
 *             C00 = Syy*n - Sy*Sy   C01 = Sx*Sy - Sxy*n   C02 = Sxy*Sy - Syy*Sx
 *             C11 = Sxx*n - Sx*Sx   C12 = Sxy*Sx - Sxx*Sy C22 = Sxx*Syy - Sxy*Sxy   det = Sxx*C00 + Sxy*C01 + Sx*C02
 *           VALID iff n >= min_support and det > 0 (a collinear or single-pixel support has det == 0 exactly); in binary64
 *             a64 = (((C00*Sxe) + (C01*Sye)) + (C02*Se)) / det,  b64 with (C01, C11, C12),  c64 with (C02, C12, C22);
 *           a = (float)a64, b = (float)b64, z = (float)((double)d0 + c64): the fitted disparity at the pixel.
 *   out     d_planes = (a, b, z) where VALID else (0, 0, 0); d_support = n, valid or not; d_normals = the normal of
 *           pm_planes_normals above for the plane (a, b, z) of pixel (x, y), (0, 0, 0) where not VALID, where z is not > 0
 *           and where its length is not finite.
 * Valid in every mode of the handle: it reads a map, not the handle's state.  Images smaller than the window are legal;
 * taps outside the image never count.  One launch; a workgroup stages its tile and an r-wide halo in LDS once.
 * PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued: a null fit or d_disp; no output at all;
 * d_normals without a camera, or with one pm_backproject refuses (the camera is read for d_normals alone); radius outside
 * 1..7; a max_diff that is not finite or < 0; min_support outside 3..(2r+1)^2; rows or cols < 1.  PM_ERR_SIZE as for
 * pm_backproject. */
typedef struct pm_normals_fit { int radius; float max_diff; int min_support; } pm_normals_fit;
int pm_disparity_normals(pm_handle* h, const pm_cloud_camera* camera, const pm_normals_fit* fit,
                         const float* d_disp, int rows, int cols,
                         float* d_normals   /* [rows][cols][3], may be NULL */,
                         float* d_planes    /* [3][rows][cols]: a, b, z, may be NULL */,
                         uint8_t* d_support /* [rows][cols], may be NULL */);

/* ---- speckle filter: the map's connected regions of similar disparity; small ones are set to 0 ------------------------
 * What it is for: between Match() and the stages above.  The cross-check and pm_remove_background leave small islands of
 * wrong disparity in weakly textured water; pm_point_cloud turns each into a cluster of floating points and
 * pm_disparity_normals fits planes through it.  The step is cv::filterSpeckles'; the labels and sizes are outputs too, since
 * a meshing consumer can use the segments.  It fills nothing and smooths nothing.  Held to its CPU definition
 * (tests/speckle_ref.py) BIT FOR BIT:
 *   valid      a pixel is valid iff d > 0: 0, -0.0, negatives and NaN are not, +inf is.
 *   edge       two 4-neighbours p, q are joined iff both are valid and fabs((double)d(p) - (double)d(q)) <= (double)max_diff
 *              in binary64.  A NaN difference never joins, so a +inf pixel is a component of its own.  No diagonals.
 *   component  the transitive closure of the edges (a slow ramp is one component, as in OpenCV).
 *   d_out      a valid pixel whose component has at most max_size pixels becomes +0.0f; every other pixel, invalid ones
 *              included, keeps its input bits.  d_out may equal d_disp.  max_size == 0 removes nothing.
 *   d_labels   the smallest linear index y * cols + x of the pixel's component, -1 where the pixel is invalid.  Labels are
 *              those of the INPUT map, removed components included.
 *   d_sizes    the component's pixel count, 0 where the pixel is invalid.
 *   removed    the number of pixels set to 0, to *d_removed (device) and *removed (host), also where d_out is NULL.
 * Every output is optional, but at least one must be given; each is a pure function of the input (across workgroups only
 * integer min and integer add are used, so nothing depends on the order in which atomics arrive).  Valid in every mode of
 * the handle: it reads a map, not the handle's state.  Images smaller than a tile, or no multiple of it, are legal.
 * A non-NULL `removed` synchronises the stream like pm_point_cloud's `count`; with removed == NULL the call only enqueues.
 * Four launches behind a 16-byte memset (label 64 x 16 tiles in LDS, unite across tile borders, flatten, apply), none of
 * which waits for another workgroup.  Scratch (8 bytes per pixel: working labels and root sizes, and 16 bytes for the count)
 * is allocated on first use, reused, and released with the handle; growing it synchronises the stream, so a size must
 * have run once before it is captured.  The serpentine-shaped worst case takes longer than a natural map.
 * PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued: a null filter or d_disp; no output at
 * all; a max_diff that is not finite or < 0; max_size < 0; rows or cols < 1.  PM_ERR_SIZE: more than 2^31 - 1 pixels. */
typedef struct pm_speckle_filter { float max_diff; int max_size; } pm_speckle_filter;
int pm_filter_speckles(pm_handle* h, const pm_speckle_filter* filter, const float* d_disp, int rows, int cols,
                       float* d_out /* may be NULL, may equal d_disp */, int32_t* d_labels /* may be NULL */,
                       int32_t* d_sizes /* may be NULL */, int* d_removed /* device, may be NULL */,
                       int* removed /* host, may be NULL */);

/* ---- grid mesh: the triangle mesh of a disparity map's stride grid, vertices and triangles compacted on the device ----
 * What it is for: the surface behind pm_point_cloud.  Every 2x2 cell of the grid becomes up to two triangles unless a depth
 * edge runs through it; the vertex streams are pm_point_cloud's.  Held to its CPU definition (tests/mesh_ref.py) BIT FOR BIT:
 *   grid       pm_cloud_filter's stride grid: sub_rows = ceil(rows / stride), sub_cols = ceil(cols / stride); item (xs, ys) is
 *              pixel (xs * stride, ys * stride) and COUNTS iff pm_point_cloud would count that pixel (d > 0, d >= min_disp,
 *              the max_range test on the point's binary32 Z).
 *   edge       two items p, q pass iff both count and fabs((double)d(p) - (double)d(q)) <= (double)max_diff in binary64:
 *              pm_filter_speckles' rule.  A NaN difference (+inf against +inf) never passes.
 *   cell       (xs, ys) with xs < sub_cols - 1 and ys < sub_rows - 1 has the corners 00 = (xs, ys), 10 = (xs + 1, ys),
 *              01 = (xs, ys + 1), 11 = (xs + 1, ys + 1); n of them count.  n == 4: diagonal 1 (10-01) iff
 *              fabs(d10 - d01) < fabs(d00 - d11) (binary64, strict; a tie or a NaN gives diagonal 0, 00-11).  n == 3:
 *              diagonal 1 if 00 or 11 is the missing corner, diagonal 0 if 10 or 01 is.  n < 3: no triangle.
 *                diagonal 0:  T0 = (00, 01, 11)  T1 = (00, 11, 10)        diagonal 1:  T0 = (00, 01, 10)  T1 = (10, 01, 11)
 *              A triangle is EMITTED iff its three corners count and its three edges pass.  In this corner order
 *              (P1 - P0) x (P2 - P0) of the points has a negative Z (fx, fy, baseline > 0): the triangle faces the camera,
 *              like the normals of pm_planes_normals.
 *   vertices   PM_MESH_VERTICES_ALL: every counting item; the vertex streams are then EXACTLY pm_point_cloud's outputs for
 *              the same arguments.  PM_MESH_VERTICES_REFERENCED: only the counting items that are a corner of an emitted
 *              triangle (a function of the item's 3x3 neighbourhood), so the mesh has no floating points.  The k-th vertex
 *              in row-major grid order gets slot k of d_xyz_out, d_normals_out, d_bgr8_out and d_index_out (y * cols + x of
 *              the pixel), as in pm_point_cloud.
 *   triangles  cells in row-major order, T0 before T1 inside a cell; the j-th emitted triangle goes to slot j of d_tri_out
 *              as three int32 vertex slots in the order above.  The set of emitted triangles does not depend on
 *              options->vertices, only their indices do.
 *   counts     counts[0] / d_counts[0] = vertices, [1] = triangles, EVEN BEYOND the capacities; exactly the first
 *              vertex_capacity vertices and tri_capacity triangles are written and nothing behind them.  Triangle indices
 *              ALWAYS use the untruncated vertex numbering: vertex_count > vertex_capacity tells the caller that written
 *              triangles may name vertices that were not written.
 * Every output is optional; both capacities may be 0 and the call then only counts.  A grid with fewer than two rows or
 * columns is legal and has no triangles.  Valid in every mode of the handle: it reads a map, not the handle's state.  It
 * enqueues on the handle's stream; a non-NULL `counts` synchronises it like pm_point_cloud's `count`.
 * Five small launches, none of which waits for another workgroup (per-block vertex and triangle counts by wavefront ballot
 * over an LDS tile of three grid rows, two launches of pm_point_cloud's offsets kernel, the vertex scatter that also writes
 * an organised slot map, the triangle scatter that reads it); the order comes from that arithmetic, never from atomics.
 * Scratch (8 bytes per 256 grid items of a row, 4 bytes per grid item for the slot map, 8 for the counts) is ONE allocation,
 * made on first use, reused, and released with the handle; growing it synchronises the stream, so a size must have run
 * once before it is captured.
 * PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued: everything pm_point_cloud refuses (with
 * either capacity < 0); null options; a max_diff that is not finite or < 0; a `vertices` outside the enum.  PM_ERR_SIZE as
 * for pm_point_cloud, and where 2 * (sub_rows - 1) * (sub_cols - 1) exceeds 2^31 - 1. */
typedef enum pm_mesh_vertices { PM_MESH_VERTICES_ALL = 0, PM_MESH_VERTICES_REFERENCED = 1 } pm_mesh_vertices;
typedef struct pm_mesh_options { float max_diff; int vertices; } pm_mesh_options;
int pm_grid_mesh(pm_handle* h, const pm_cloud_camera* camera, const pm_cloud_filter* filter,
                 const pm_mesh_options* options, const float* d_disp,
                 const float* d_normals /* organised, may be NULL */, const uint8_t* d_bgr8 /* may be NULL */,
                 int rows, int cols, int vertex_capacity, int tri_capacity,
                 float* d_xyz_out, float* d_normals_out, uint8_t* d_bgr8_out, int32_t* d_index_out,
                 int32_t* d_tri_out /* [tri_capacity][3], may be NULL */,
                 int* d_counts /* device int[2]: vertices, triangles; may be NULL */,
                 int* counts /* host int[2]; may be NULL; non-NULL synchronises like pm_point_cloud's count */);

/* ---- temporal seeds: the left map of frame k carried into the two seed maps of frame k + 1 --------------------------------
 * What it is for: the link between two frames of a sequence.  The d_seed_l / d_seed_r inputs of every Match entry point take a
 * value > 0 as the start of that pixel and 0 as background; this stage makes both maps on the device from the OLD frame's left
 * disparity map and the rigid motion between the two left cameras (from a VIO front end), the classic temporal PatchMatch
 * step.  With R = I and t = 0 it is "reuse the last map" for a static camera, and it still produces the right-view map.
 * Held to its CPU definition (tests/reproject_ref.py) BIT FOR BIT:
 *   motion     X_new = R X_old + t between the LEFT camera frames, R row-major.  From two poses of the left camera in a
 *              world frame: T_new_old = T_world_new^-1 * T_world_old.  R is NOT checked for orthonormality: the arithmetic
 *              below is defined for any finite R and t.
 *   splat      a source pixel (x, y) with value d takes part iff d > 0 and d >= min_disp (binary32: never for NaN).  In
 *              binary64, fxB = fx * baseline formed once:  Z = fxB / (double)d;  X = (((double)x - cx) * Z) / fx;
 *              Y = (((double)y - cy) * Z) / fy  (pm_backproject's values before their rounding);
 *              Xn = (((R0*X) + (R1*Y)) + (R2*Z)) + t0;  Yn with R3..R5 and t1;  Zn with R6..R8 and t2;  dropped unless
 *              Zn > 0;  dn = (float)(fxB / Zn), dropped unless dn > 0 and finite, and unless dn <= max_disp where
 *              max_disp != 0;  u = (fx * (Xn / Zn)) + cx;  v = (fy * (Yn / Zn)) + cy;  dropped unless |u| < 2^30 and
 *              |v| < 2^30;  iu = rint(u), iv = rint(v), half to even;  dropped unless 0 <= iu < cols and 0 <= iv < rows.
 *              S_l(iv, iu) = the binary32 maximum of dn over every source pixel that lands there: the nearest surface wins.
 *              Pixels nobody lands on are +0.0.
 *   close      C(y, x) = S(y, x) where S(y, x) > 0; elsewhere the maximum of S over the (2r+1)^2 window, r = close_radius,
 *              taps outside the image not counting, 0 if no tap is > 0.  r = 0 copies.  It closes the one-pixel cracks a
 *              forward splat leaves when the camera advances or turns and never alters a pixel that was hit.
 *   right      from the CLOSED left seed C_l: every (x, y) with s = C_l(y, x) > 0 gives q = rint((double)x - (double)s),
 *              dropped unless 0 <= q < cols;  S_r(y, q) = the maximum of s over its contributors, else +0.0 -- a map in
 *              right-image coordinates, the convention pm_mask_occlusions reads.  Then the same close with the same r.
 *   counts     counts[0] / d_counts[0] = pixels > 0 of C_l (d_seed_l), [1] = pixels > 0 of C_r (d_seed_r).
 * At least one of d_seed_l, d_seed_r, d_counts, counts must be given; d_seed_r alone is legal (the left seed then lives in
 * scratch only).  d_seed_l and d_seed_r must not alias d_disp.  Valid in every mode of the handle: it reads a map, not the
 * handle's state.  It enqueues on the handle's stream; a non-NULL `counts` synchronises it like pm_point_cloud's `count`,
 * otherwise the call only enqueues.  pm_submit_device is NOT ordered behind the handle's stream: record an event on
 * pm_stream(h) behind this call and hand it to pm_submit_device_after with the two seed maps.
 * One memset and four launches, none of which waits for another workgroup (the splat with one integer atomicMax per
 * surviving pixel, close + count over an LDS tile with an r-wide halo, the right splat, close + count again); only integer
 * maximum and integer addition cross workgroups, so the result does not depend on the order of arrival.  Scratch (two maps
 * of 4 bytes per pixel and the counts; a third map where d_seed_l is NULL) is ONE allocation, made on first use, reused, and
 * released with the handle; growing it synchronises the stream, so a size must have run once before it is captured.
 * PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued: a null camera, motion, options or d_disp;
 * a camera pm_backproject refuses; a non-finite entry of R or t; a NaN or negative min_disp / max_disp; a close_radius
 * outside 0..3; rows or cols < 1; no output at all; an output equal to d_disp.  PM_ERR_SIZE as for pm_backproject. */
typedef struct pm_motion { double R[9]; double t[3]; } pm_motion;   /* X_new = R X_old + t, left camera frames */
typedef struct pm_reproject_options { float min_disp; float max_disp; int close_radius; } pm_reproject_options;
int pm_reproject_disparity(pm_handle* h, const pm_cloud_camera* camera, const pm_motion* motion,
                           const pm_reproject_options* options, const float* d_disp, int rows, int cols,
                           float* d_seed_l /* may be NULL */, float* d_seed_r /* may be NULL */,
                           int* d_counts /* device int[2], may be NULL */, int* counts /* host int[2], may be NULL */);

/* ---- geometric consistency: keep of a map what earlier frames of the sequence confirm ------------------------------------
 * What it is for: the judgement a sequence can pass on a map.  PatchMatch's mistakes follow per-frame noise, so a wrong island
 * of frame k is usually elsewhere in frame k - 1.  Every pixel of the CURRENT left map is carried into n earlier left maps of
 * the same size and rectified camera through the known motions (the geometric consistency check of multi-view PatchMatch with
 * visibility-based fusion): it is kept iff enough of them saw the same surface and not too many saw through it.  The depth is
 * known in the current frame, so every lookup is a gather; nothing is averaged or filled.
 * Held to its CPU definition (tests/consistency_ref.py) BIT FOR BIT:
 *   motions    motions[k]: X_src_k = R X_cur + t between the LEFT camera frames, R row-major: with pm_reproject_disparity's
 *              convention, the motion from the current pose (as "old") to source k's pose (as "new").
 *   valid      a current pixel is valid iff d = D(y, x) > 0 (binary32): not for 0, -0.0, negatives and NaN; +inf is valid.
 *   project    into source k: EXACTLY pm_reproject_disparity's `splat` arithmetic with min_disp = 0 and max_disp = 0 (Z, X, Y;
 *              Xn, Yn, Zn, dropped unless Zn > 0; dp = (float)(fxB / Zn), dropped unless dp > 0 and finite; u, v, the 2^30
 *              guard, rint half to even, dropped outside the image) -> (iu, iv) and dp.  A dropped pixel has class UNSEEN.
 *   tap        the window dy = -radius..radius, dx = -radius..radius around (iu, iv) in row-major order; a tap COUNTS iff it
 *              lies inside the image and ds = D_k(iv + dy, iu + dx) > 0; e = (double)ds - (double)dp in binary64.  The chosen
 *              tap is the FIRST one with the smallest fabs(e): a later tap replaces it only with a strictly smaller value (a
 *              ds of +inf gives e = +inf and loses against any finite one).  No counting tap: class UNSEEN.
 *   class      with md = (double)max_diff:  fabs(e) <= md  CONSISTENT (1);  e > md  OCCLUDED (2): the source saw something
 *              nearer there and says nothing about this pixel;  e < -md  CONFLICT (3): the source saw through the point;
 *              UNSEEN is 0.
 *   per pixel  n_cons, n_conf: the sources of class 1 and of class 3.  S: a binary64 sum from +0.0 over k = 0 .. n - 1 in
 *              order, S = S + fabs(e_k) for the CONSISTENT sources.  KEPT iff valid, n_cons >= min_consistent and
 *              n_conf <= max_conflicts.
 *   d_out      a valid pixel that is not KEPT becomes +0.0f; every other pixel, invalid ones included, keeps its input bits
 *              (pm_filter_speckles' rule).  May equal d_disp unless d_disp is itself a source.
 *   d_classes  uint16 per pixel: the class of source k in bits 2k and 2k + 1; 0 for an invalid pixel.
 *   d_residual (float)(S / (double)n_cons), +0.0 where n_cons == 0 or the pixel is invalid.
 *   counts     counts[0] / d_counts[0] = valid pixels, [1] = kept pixels.
 * Every output is optional, but at least one must be given.  A source may be d_disp itself.  Valid in every mode of the
 * handle: it reads maps, not the handle's state.  It enqueues on the handle's stream; a non-NULL `counts` synchronises it like
 * pm_point_cloud's `count`, otherwise the call only enqueues.  d_sources and motions are HOST arrays of n_sources entries,
 * read before the call returns.  One launch behind a 16-byte memset; only integer addition crosses workgroups, so every output
 * is a pure function of the inputs.  Scratch is the 16 bytes of the counts, allocated on first use, reused, and released with
 * the handle.
 * PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued: a null camera, options, d_disp, d_sources,
 * motions or d_sources[k]; a camera pm_backproject refuses; n_sources outside 1..PM_CONSISTENCY_MAX_SOURCES; a non-finite
 * entry of motions[k] (named with k); a max_diff that is not finite or < 0; radius outside 0..2; min_consistent outside
 * 0..n_sources; max_conflicts outside 0..8; rows or cols < 1; no output at all; d_out equal to a source (this covers
 * d_out == d_disp where d_disp is itself a source).  PM_ERR_SIZE as for pm_backproject. */
#define PM_CONSISTENCY_MAX_SOURCES 8
enum { PM_CONSISTENCY_UNSEEN = 0, PM_CONSISTENCY_CONSISTENT = 1, PM_CONSISTENCY_OCCLUDED = 2, PM_CONSISTENCY_CONFLICT = 3 };
typedef struct pm_consistency_options { float max_diff; int radius; int min_consistent; int max_conflicts; } pm_consistency_options;
int pm_filter_consistency(pm_handle* h, const pm_cloud_camera* camera, const pm_consistency_options* options,
                          const float* d_disp, int n_sources, const float* const* d_sources /* host array of device maps */,
                          const pm_motion* motions /* host array */, int rows, int cols,
                          float* d_out /* may be NULL, may equal d_disp */, uint16_t* d_classes /* may be NULL */,
                          float* d_residual /* may be NULL */, int* d_counts /* device int[2], may be NULL */,
                          int* counts /* host int[2], may be NULL: non-NULL synchronises like pm_point_cloud's count */);

/* ---- matching confidence: how well each disparity of a map matched ----------------------------------------------------------
 * What it is for: every stage behind Match() treats each positive disparity as equally good.  PatchMatch keeps no cost volume,
 * so this stage evaluates the matching functor again around the answer -- at d, one pixel either side of d, and at the
 * background hypothesis d = 0 (the comparison RemoveBackground makes) -- and, where the right map is given, reads the
 * left-right residual.  It returns the four measures, a flag byte per pixel and the map with the failing pixels zeroed; a
 * consumer thresholds a cloud, weights a fusion or keeps only trustworthy temporal seeds.  It sits behind Match() and in front
 * of pm_filter_speckles.
 * Held to its CPU definition (tests/confidence_ref.py) BIT FOR BIT.  G_l, G_r are the Sobel magnitudes of the two images
 * (pm_gradient_magnitude); cost(x, y, d) is the PM_SEM_CPU cost of the patch_w x patch_h window at (x, y) under the handle's
 * functor_alpha, functor_tau_color, functor_tau_grad -- always that functor, whatever the handle's semantics or mode.  Every
 * operation is one binary32 rounding unless it says binary64:
 *   interior   pw / 2 <= x <= cols - pw / 2 - 1 and ph / 2 <= y <= rows - ph / 2 - 1 (empty where the window does not fit).
 *   valid      d = D_l(y, x) > 0: not for 0, -0.0, negatives and NaN.
 *   MEASURED   valid, interior and d <= hi with hi = (float)x - (float)(pw / 2): the domain in which the window stays in the
 *              image; every interior value Match() returns lies in it.  +inf and values beyond hi are valid but not measured;
 *              nothing is clamped.
 *   costs      c0 = cost(d); c_bg = cost(+0.0f); dm = d - 1.0f, side M exists iff dm >= 0, cm = cost(dm); dp = d + 1.0f, side P
 *              exists iff dp <= hi, cp = cost(dp).
 *   margin     both sides: (cp < cm ? cp : cm) - c0; one side: that side's cost - c0; none: +0.0f.  Negative: d is not even a
 *              local minimum.
 *   bg_margin  c_bg - c0.
 *   lr         with d_disp_r: q = (int)fmaxf((float)x - d, 0.f) (pm_mask_occlusions' index), r = D_r(y, q); r > 0:
 *              (float)fabs((double)r - (double)d) in binary64, otherwise +inf.  Without d_disp_r: +inf.
 *   flags      a measured pixel: PM_CONF_MEASURED plus one PM_CONF_FAIL_* bit per threshold it does not PASS (see the struct;
 *              a +inf lr passes only max_lr_diff = +inf; FAIL_LR only ever with d_disp_r).  Not measured: 0.  KEPT iff
 *              flags == PM_CONF_MEASURED.
 *   d_out      a measured pixel that is not KEPT becomes +0.0f; with drop_unmeasured = 1 so does a valid pixel that is not
 *              measured; every other pixel, invalid ones included, keeps its input bits (pm_filter_speckles' rule).  May equal
 *              d_disp_l.
 *   d_measures four planes c0, margin, bg_margin, lr; a pixel that is not measured gets -1.0f, +0.0f, +0.0f, +inf.
 *   counts     [0] valid, [1] measured, [2] kept pixels.
 * Every output is optional, but at least one must be given.  Valid in every mode of the handle: it reads images and maps, not
 * the handle's state.  It enqueues on the handle's stream; a non-NULL `counts` synchronises it like pm_point_cloud's `count`.
 * Two launches behind a 16-byte memset; only integer addition crosses workgroups.  Scratch is one allocation (16 bytes of counts,
 * a byte and a float per pixel for the gradients), made on first use, reused, grown under a stream synchronisation and
 * released with the handle.
 * PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued: null options, d_left, d_right or d_disp_l;
 * no output at all; patch_w or patch_h even or outside 3..PM_MAX_PATCH; a NaN threshold; drop_unmeasured outside {0, 1}; rows
 * or cols < 1; d_out equal to d_disp_r.  PM_ERR_SIZE as for pm_backproject. */
typedef struct pm_confidence_options {
  int   patch_w, patch_h;   /* odd, 3 .. PM_MAX_PATCH each; need not be square                    */
  float max_cost;           /* PASS iff c0 <= max_cost;              +inf: every pixel passes      */
  float min_margin;         /* PASS iff margin >= min_margin;        -inf: every pixel passes      */
  float min_bg_margin;      /* PASS iff bg_margin >= min_bg_margin;  -inf: every pixel passes      */
  float max_lr_diff;        /* PASS iff lr <= max_lr_diff;           +inf: every pixel passes;
                               read only when d_disp_r is given                                   */
  int   drop_unmeasured;    /* 0 / 1, see d_out                                                    */
} pm_confidence_options;
enum { PM_CONF_MEASURED = 1, PM_CONF_FAIL_COST = 2, PM_CONF_FAIL_MARGIN = 4, PM_CONF_FAIL_BG = 8, PM_CONF_FAIL_LR = 16 };
int pm_disparity_confidence(pm_handle* h, const pm_confidence_options* options,
                            const uint8_t* d_left, const uint8_t* d_right,      /* rectified, [rows][cols], packed */
                            const float* d_disp_l, const float* d_disp_r /* may be NULL */, int rows, int cols,
                            float* d_out      /* may be NULL, may equal d_disp_l */,
                            float* d_measures /* [4][rows][cols]: c0, margin, bg_margin, lr; may be NULL */,
                            uint8_t* d_flags  /* [rows][cols], may be NULL */,
                            int* d_counts     /* device int[3], may be NULL */,
                            int* counts       /* host int[3], may be NULL: non-NULL synchronises like pm_point_cloud's count */);

/* ---- sequence fusion: the newest left map refined by, and filled from, earlier maps of the sequence ---------------------------
 * What it is for: pm_reproject_disparity carries a map forward and pm_filter_consistency removes what earlier frames
 * contradict; neither improves a value or recovers a lost one.  The per-frame noise of a PatchMatch map is independent between
 * frames, so this stage averages, per pixel of the CURRENT left map, the observations the n earlier left maps made of the same
 * surface (visibility-based fusion of multi-view PatchMatch), and gives a pixel that lost its value in this frame (cross-check,
 * background mask, confidence filter) the value the earlier frames agree on.  It sits behind pm_disparity_confidence and in
 * front of pm_filter_speckles / pm_point_cloud / pm_grid_mesh.
 * Held to its CPU definition (tests/fuse_ref.py) BIT FOR BIT.  Binary64 unless it says binary32, one rounding per operation,
 * parentheses as written; fxB = fx * baseline formed once:
 *   motions    pm_filter_consistency's: motions[k] is X_src_k = R X_cur + t between the LEFT camera frames.
 *   refine     every valid pixel (d = D(y, x) > 0) is carried into each source with EXACTLY pm_filter_consistency's project, tap
 *              and class (max_diff, radius).  Z = fxB / (double)d and Zn are the values `project` formed.  A CONSISTENT source
 *              k, with ds the chosen tap's value, observes   Zs = fxB / (double)ds;  g = Zn - t2;  Zo = ((Zs - t2) * Z) / g;
 *              o_k = fxB / Zo   -- Zo is the depth along the pixel's own ray at which source k would have measured ds (Zn is
 *              affine in Z along a ray; no inverse motion is needed).  It TAKES PART iff g > 0, Zo > 0, o_k is finite and its
 *              weight is > 0; otherwise the source counts for its class and contributes nothing.
 *   weights    optional float planes, d_weight for the current map and d_source_weights[k] per source, the latter read at the
 *              chosen tap; a NULL plane (or a NULL d_source_weights) is 1.0 everywhere.  w counts as (double)w iff it is
 *              finite and > 0; 0, negatives, NaN and +-inf are 0 and that observation does not take part -- the margin plane
 *              of pm_disparity_confidence's d_measures can be passed as it is.
 *   sums       num = w0 * (double)d, den = w0; then over k = 0 .. n - 1 in order, the sources that take part:
 *              num = num + (w_k * o_k), den = den + w_k.  omin / omax over (double)d where w0 > 0 and the o_k that take part.
 *   KEPT       pm_filter_consistency's rule: valid, n_cons >= min_consistent, n_conf <= max_conflicts (min_consistent = 0
 *              with max_conflicts = 8 removes nothing).
 *   d_out      valid, not KEPT: +0.0f, and it is never filled;  KEPT and den > 0: (float)(num / den);  KEPT otherwise: the
 *              input bits.  May equal d_disp unless d_disp is itself a source.
 *   d_count    uint8: the observations that took part, the pixel's own included where w0 > 0: 0 .. 9.
 *   d_spread   (float)(omax - omin), +0.0 where d_count is 0.
 *   NaN        a quotient or difference that is NaN (only a valid pixel that is +inf makes one) is stored as 0x7FC00000.
 *   fill       only with fill_min_sources >= 1; with 0 an invalid pixel keeps its input bits and no splat runs.  The inverse
 *              of motions[k] is formed on the host:  Rinv[3i+j] = R[3j+i];  tinv_i = -(((R[i]*t0) + (R[3+i]*t1)) + (R[6+i]*t2))
 *              (R is still not checked).  S_k is EXACTLY pm_reproject_disparity's `splat` of source k through (Rinv, tinv) with
 *              min_disp = max_disp = 0 and no close: the nearest surface wins.  At an invalid pixel (d not > 0: 0, -0.0,
 *              negatives, NaN):  c_k = S_k(y, x) is a candidate iff c_k > 0;  m = the binary32 maximum of the candidates;
 *              source k SUPPORTS iff c_k > 0 and fabs((double)c_k - (double)m) <= (double)fill_max_diff;  FILLED iff the
 *              number of supporters n_sup >= fill_min_sources;  then acc from +0.0 in k order over the supporters,
 *              acc = acc + (double)c_k;  d_out = (float)(acc / (double)n_sup);  d_count = n_sup;
 *              d_spread = (float)((double)m - (double)(the smallest supporter)).  An invalid pixel that is not filled keeps its
 *              input bits (pm_filter_speckles' rule), with d_count 0 and d_spread +0.0.  Weights play no part in a fill: a
 *              caller who distrusts a source's pixels passes that source already filtered.
 *   d_flags    uint8: PM_FUSE_VALID, PM_FUSE_KEPT, PM_FUSE_FUSED (kept, and at least one SOURCE observation took part),
 *              PM_FUSE_FILLED.
 *   counts     [0] valid, [1] kept, [2] fused, [3] filled pixels.
 * Every output is optional, but at least one must be given.  A source may be d_disp itself.  Valid in every mode of the
 * handle: it reads maps, not the handle's state.  It enqueues on the handle's stream; a non-NULL `counts` synchronises it like
 * pm_point_cloud's `count`, otherwise the call only enqueues.  d_sources, motions and d_source_weights are HOST arrays of
 * n_sources entries, read before the call returns.  One memset and one launch, two launches when filling; only integer maximum
 * and integer addition cross workgroups, so every output is a pure function of the inputs.  Scratch (16 bytes of counts and,
 * when filling, n_sources maps of 4 bytes per pixel) is ONE allocation, made on first use, reused, grown under a stream
 * synchronisation and released with the handle, so a size must have run once before it is captured.
 * PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued: everything pm_filter_consistency refuses;
 * fill_min_sources outside 0..n_sources; a fill_max_diff that is not finite or < 0; d_out, d_count, d_spread or d_flags equal
 * to a source or to a source's weight plane.  PM_ERR_SIZE as for pm_backproject. */
enum { PM_FUSE_VALID = 1, PM_FUSE_KEPT = 2, PM_FUSE_FUSED = 4, PM_FUSE_FILLED = 8 };
typedef struct pm_fuse_options {
  float max_diff; int radius; int min_consistent; int max_conflicts;   /* pm_consistency_options' four          */
  int   fill_min_sources;                                              /* 0: no fill; else 1 .. n_sources       */
  float fill_max_diff;                                                 /* finite, >= 0                          */
} pm_fuse_options;
int pm_fuse_disparity(pm_handle* h, const pm_cloud_camera* camera, const pm_fuse_options* options,
                      const float* d_disp, const float* d_weight /* may be NULL */, int n_sources,
                      const float* const* d_sources /* host array of device maps */, const pm_motion* motions /* host array */,
                      const float* const* d_source_weights /* host array, may be NULL, entries may be NULL */,
                      int rows, int cols,
                      float* d_out /* may be NULL, may equal d_disp */, uint8_t* d_count /* may be NULL */,
                      float* d_spread /* may be NULL */, uint8_t* d_flags /* may be NULL */,
                      int* d_counts /* device int[4], may be NULL */,
                      int* counts /* host int[4], may be NULL: non-NULL synchronises like pm_point_cloud's count */);

/* ---- camera motion between two frames of a sequence ---------------------------------------------------------------------------
 * What it is for: pm_reproject_disparity, pm_filter_consistency and pm_fuse_disparity take the rigid motion of the left camera
 * as an input.  When frame k + 1 arrives, everything an estimate of it needs is on the device: the left image of frame k, its
 * disparity map (a 3-D point per pixel) and the left image of frame k + 1.  pm_track_features picks one corner per cell of the
 * old image, predicts where each lands in the new image under a guess of the motion, and finds it there by block matching;
 * pm_solve_motion (host, binary64) fits the motion to the tracks by Gauss-Newton on the reprojection error with Huber weights;
 * pm_estimate_motion runs both.  The motion is pm_reproject_disparity's: X_new = R X_old + t between the left camera frames,
 * and can be handed to that stage unchanged.
 * Held to its CPU definition (tests/motion_ref.py) BIT FOR BIT; the kernels select and match in exact integer arithmetic:
 *   score      gx, gy: the 3x3 Sobel responses of the old image; Sxx, Syy, Sxy: sums of gx gx, gy gy, gx gy over the 7x7 window;
 *              score = 16 (Sxx Syy - Sxy Sxy) - (Sxx + Syy)^2 in int64 (Harris with k = 1/16).
 *   eligible   m = max(p, 4); m <= x <= cols - 1 - m, m <= y <= rows - 1 - m; d = D_old(y, x) finite, > 0, >= min_disp, and
 *              <= max_disp where max_disp != 0; score >= min_score.
 *   select     cell (cx, cy) covers x in [cx cell, min(cols, (cx + 1) cell)), y likewise; its feature is the eligible pixel of
 *              the largest score, a tie going to the smallest y cols + x.  Features are numbered by cell, row-major: the k-th
 *              feature is record k.
 *   predict    pm_reproject_disparity's `splat` arithmetic through the guess: Z, X, Y; Xn, Yn, Zn; u, v; PREDICTED iff Zn > 0
 *              and |u|, |v| < 2^30; (iu, iv) = rint, half to even, and may lie outside the image.  A record that is not
 *              predicted has x_new = y_new = 0, sad = second = INT32_MAX and no flag.
 *   match      candidates (qx, qy) = (iu + ex, iv + ey), ey and ex in -s .. s, row-major; a candidate COUNTS iff its (2p+1)^2
 *              patch lies inside the new image; SAD over the patch; the best is the first of the smallest SAD; MATCHED iff a
 *              candidate counts; `second`: the smallest SAD of a counting candidate at Chebyshev distance >= 2 from the best.
 *              A predicted record without a counting candidate has x_new = (float)iu, y_new = (float)iv, sad = second =
 *              INT32_MAX and PREDICTED alone.
 *   sub-pixel  in x: iff (qx - 1, qy) and (qx + 1, qy) are candidates of the window that count, den = cm - 2 c0 + cp > 0 and
 *              c0 > 0 (a perfect match stays on its pixel): x_new = (float)((double)qx + (double)(cm - cp) / (double)(2 den))
 *              and SUBPIX_X; otherwise (float)qx.  Same in y.
 *   OK         flags & (PREDICTED | MATCHED | FAIL_SAD | FAIL_GAP) == PREDICTED | MATCHED: the tracks the solve uses.
 *   solve      binary64, one rounding per operation, in the order tests/motion_ref.py writes out.  P_i: pm_backproject's point of
 *              (x, y, disp) before its rounding.  Per iteration, over the OK tracks in order from +0.0: Q = R P + t, skipped
 *              unless Qz > 0; iz = 1 / Qz; a = Qx iz; b = Qy iz; ru = ((fx a) + cx) - x_new; rv likewise; e = sqrt(ru ru + rv rv);
 *              w = 1 if e <= huber_px, else huber_px / e; J for the left perturbation Q' = Q + omega x Q + upsilon, delta =
 *              (omega, upsilon); H += w J^T J, g += w J^T r; H delta = -g by LDL^T without pivoting, which fails iff a pivot is
 *              not > 0; the Cayley update with a = omega / 2: dR = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a), R <- dR R,
 *              t <- dR t + upsilon; it stops after the update when max |delta_i| < epsilon, or after `iterations`.  Under the
 *              motion reached: n_used (Qz > 0), the inliers (e <= inlier_px) and their root-mean-square e.  info->iterations:
 *              the updates made; info->n_tracks: the OK tracks.  valid iff no factorisation failed and n_inliers >= min_inliers.
 * No new status code: a solve that cannot be trusted returns PM_OK with info->valid == 0 and *out equal to the guess.
 * pm_track_features enqueues on the handle's stream and is valid in every mode of the handle.  count, d_count and capacity
 * behave as pm_point_cloud's: the count (the number of features) is reported beyond the capacity, exactly the first `capacity`
 * records are written, capacity == 0 only counts, a non-NULL `count` synchronises the stream.  pm_estimate_motion tracks into
 * scratch of the handle, downloads the records and solves; it always synchronises.  pm_solve_motion needs no handle, and its
 * status alone reports a refusal.  Scratch (16 bytes, two words per cell and, for pm_estimate_motion, one record per cell) is
 * ONE allocation, made on first use, reused, grown under a stream synchronisation and released with the handle.
 * PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued: a null required pointer; a camera that
 * pm_backproject refuses; a non-finite entry of the guess; an option outside its range below, NaN thresholds included; rows or
 * cols < 1; no output at all; capacity < 0.  PM_ERR_SIZE as for pm_backproject. */
typedef struct pm_track {            /* 32 bytes */
  int32_t x, y;                      /* the feature's pixel in the OLD left image          */
  float   disp;                      /* D_old(y, x)                                        */
  float   x_new, y_new;              /* its position in the NEW left image, sub-pixel      */
  int32_t sad, second;               /* best SAD; best SAD at Chebyshev distance >= 2 from it, INT32_MAX if none */
  uint32_t flags;                    /* PM_TRACK_* */
} pm_track;
enum { PM_TRACK_PREDICTED = 1, PM_TRACK_MATCHED = 2, PM_TRACK_SUBPIX_X = 4, PM_TRACK_SUBPIX_Y = 8,
       PM_TRACK_FAIL_SAD = 16, PM_TRACK_FAIL_GAP = 32 };
typedef struct pm_track_options {
  int cell;            /* 8..64: one feature per cell x cell pixels                         */
  int patch_radius;    /* p, 1..7                                                           */
  int search_radius;   /* s, 0..24                                                          */
  int64_t min_score;   /* >= 1                                                              */
  float min_disp, max_disp;  /* as pm_reproject_options; max_disp 0 = no limit             */
  int max_sad;         /* >= 0, 0 = no limit: FAIL_SAD iff sad > max_sad                    */
  int min_gap;         /* >= 0: FAIL_GAP iff second - sad < min_gap (second = INT32_MAX never fails) */
} pm_track_options;
typedef struct pm_solve_options { int iterations /*1..50*/; double huber_px /*>0*/; double epsilon /*>=0*/;
                                  double inlier_px /*>0*/; int min_inliers /*>=6*/; } pm_solve_options;
typedef struct pm_motion_info { int valid, n_tracks, n_used, n_inliers, iterations; double rms_px; } pm_motion_info;

int pm_track_features(pm_handle* h, const pm_cloud_camera* camera, const pm_track_options* options,
                      const pm_motion* guess /* NULL = identity */, const uint8_t* d_left_old, const float* d_disp_old,
                      const uint8_t* d_left_new, int rows, int cols, int capacity, pm_track* d_tracks /* may be NULL */,
                      int* d_count /* may be NULL */, int* count /* host, may be NULL: non-NULL synchronises */);
int pm_solve_motion(const pm_cloud_camera* camera, const pm_solve_options* options, const pm_track* tracks /* host */, int n,
                    const pm_motion* guess /* NULL = identity */, pm_motion* out /* may be NULL */,
                    pm_motion_info* info /* may be NULL */);      /* host only, no handle */
int pm_estimate_motion(pm_handle* h, const pm_cloud_camera* camera, const pm_track_options* track_options,
                       const pm_solve_options* solve_options, const pm_motion* guess /* NULL = identity */,
                       const uint8_t* d_left_old, const float* d_disp_old, const uint8_t* d_left_new, int rows, int cols,
                       pm_motion* out /* may be NULL */, pm_motion_info* info /* may be NULL */);

/* ---- a persistent world-frame model: a truncated signed distance volume, integrated from maps and raycast back -----------------
 * What it is for: the sequence stages above work on a sliding window of at most PM_CONSISTENCY_MAX_SOURCES earlier maps, and
 * every output lives in one camera frame.  A TSDF volume holds what the whole sequence saw, in the WORLD frame: pm_tsdf_integrate
 * folds one disparity map and its camera pose into it, pm_tsdf_raycast renders it back as an ordinary LEFT disparity map (and
 * normals) at any pose.  Every stage above consumes that map unchanged: pm_point_cloud / pm_grid_mesh make the fused surface,
 * pm_reproject_disparity with the identity motion makes the right seed, pm_submit_device_after takes the pair as seeds without
 * cracks, pm_filter_consistency / pm_fuse_disparity take it as ONE source that stands for the whole history.
 * The caller owns the volume: nx * ny * nz records of 8 bytes {float tsdf; float weight}, x fastest, in device memory
 * (pm_device_malloc, pm_tsdf_bytes); weight == 0 means never observed.  pose: X_cam = R X_world + t (a pm_motion from the world
 * frame into the left camera's).
 * Held to its CPU definition (tests/tsdf_ref.py) BIT FOR BIT.  Binary64 unless it says binary32, one rounding per operation,
 * parentheses as written; fxB = fx * baseline formed once:
 *   integrate, per voxel (i, j, k), independent of every other voxel:
 *     point    Xw = origin[0] + ((double)i * voxel); Yw, Zw likewise with j, k.
 *     project  EXACTLY pm_reproject_disparity's `splat` arithmetic from its motion line on, with max_disp = 0:
 *              Xc = (((R0*Xw) + (R1*Yw)) + (R2*Zw)) + t0; Yc, Zc likewise; dropped unless Zc > 0; dropped unless
 *              (float)(fxB / Zc) is > 0 and finite; u = (fx * (Xc / Zc)) + cx; v likewise; the 2^30 guard; rint half to even;
 *              dropped outside the rows x cols image -> (iu, iv).  A voxel that gets this far is IN VIEW.
 *     measure  d = D(iv, iu) counts iff d > 0 and d >= min_disp (binary32; never NaN).  Zm = fxB / (double)d; dropped if
 *              max_range != 0 and (float)Zm > max_range.  sdf = Zm - Zc, the projective distance along the optical axis;
 *              dropped if sdf < -trunc.  f = (float)fmin(1.0, sdf / trunc): free space in front of the surface is carved with 1.
 *     weight   wn = 1.0f, or W(iv, iu) where d_weight is given, under pm_fuse_disparity's rule: with 0, -0.0, negatives, NaN
 *              and +-inf the observation does not take part.
 *     update   binary32:  tsdf' = ((tsdf * w) + (f * wn)) / (w + wn);  w' = fminf(w + wn, max_weight).  A voxel that was
 *              dropped keeps its bits and is neither read nor written.
 *     counts   [0] voxels in view, [1] voxels updated.
 *   raycast, per pixel (x, y):
 *     inverse  formed on the host, as pm_fuse_disparity forms its inverse motions:  Ri[3i+j] = R[3j+i];
 *              c_i = -(((R[i]*t0) + (R[3+i]*t1)) + (R[6+i]*t2))  (R is not checked for being a rotation).
 *     ray      dx = ((double)x - cx) / fx; dy = ((double)y - cy) / fy; the direction in the camera frame is (dx, dy, 1), so the
 *              ray parameter s is the camera depth Z.  In the world frame wd_i = ((Ri[3i]*dx) + (Ri[3i+1]*dy)) + Ri[3i+2].
 *     samples  ds = (double)step * trunc; s_n = (double)min_range + ((double)n * ds), never accumulated, for n = 0, 1, ... while
 *              s_n <= (double)max_range.  Grid coordinates q_i = ((c_i + (s * wd_i)) - origin[i]) / voxel.
 *     sample   b_i = floor(q_i); fr_i = (float)(q_i - b_i).  VALID iff 0 <= b_i and b_i + 1 <= n_i - 1 on every axis and each
 *              of the eight corners takes part: weight > 0 and weight >= min_weight.  With lerp(a, b, t) = a + (t * (b - a)) in
 *              binary32 and T(i, j, k) the corner's tsdf:  x00 = lerp(T(b0, b1, b2), T(b0+1, b1, b2), fr0);  x10: row b1 + 1;
 *              x01: slice b2 + 1;  x11: both;  y0 = lerp(x00, x10, fr1);  y1 = lerp(x01, x11, fr1);  value = lerp(y0, y1, fr2).
 *     hit      the first n with sample n - 1 VALID and f_prev > 0, and sample n VALID and f_cur <= 0:
 *              s* = s_(n-1) + (ds * ((double)f_prev / ((double)f_prev - (double)f_cur))).  A VALID f_prev < 0 followed by a
 *              VALID f_cur > 0 is a back face and ends the ray without a hit.  A sample that is not VALID forgets f_prev.
 *     d_disp_out     (float)(fxB / s*), +0.0f without a hit.
 *     d_normals_out  q* = the grid coordinates at s*.  Along each grid axis i the sample at q* + e_i and at q* - e_i (one
 *              voxel either side); G_i = v_plus - v_minus in binary32; (0, 0, 0) where one of the six is not VALID or there is
 *              no hit.  m_i = ((R[3i]*(double)G0) + (R[3i+1]*(double)G1)) + (R[3i+2]*(double)G2); n_i = (float)m_i;
 *              normalised as pm_planes_normals does (binary32 sum of squares, sqrtf, (0, 0, 0) unless the length is finite and
 *              > 0), and negated iff ((m0*dx) + (m1*dy)) + m2 > 0, so that it faces the camera.
 *     counts   [0] pixels hit.
 * pm_tsdf_bytes needs no handle.  The other three enqueue on the handle's stream and are valid in every mode of the handle; a
 * non-NULL host `counts` synchronises like pm_point_cloud's `count`.  pm_tsdf_clear is one memset; integrate and raycast are one
 * launch each behind a 16-byte memset; no voxel is touched by two threads and only integer addition crosses workgroups, so every
 * output is a pure function of the inputs.  Scratch is the 16 bytes of the counts, allocated on first use, reused, and released
 * with the handle.
 * PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued: a null camera, volume, pose, options, d_disp
 * or d_voxels; a camera pm_backproject refuses; a non-finite entry of the pose; nx, ny, nz, rows or cols < 1; a voxel, trunc or
 * max_weight that is not finite or not > 0; a non-finite origin; integrate: a min_disp that is NaN or < 0, a max_range that is
 * not >= 0 (0 = no limit); raycast: a step outside (0, 1], ranges that are not finite or not 0 < min_range < max_range, a
 * min_weight that is NaN or < 0, no output at all (d_disp_out, d_normals_out, d_counts and counts all NULL).  PM_ERR_SIZE:
 * nx * ny * nz > 2^31 - 1; more pixels than pm_backproject takes; raycast: more than 65536 samples along a ray. */
typedef struct pm_tsdf_volume {
  int nx, ny, nz;          /* voxels; x fastest in memory                                    */
  double origin[3];        /* world position of the centre of voxel (0, 0, 0)                */
  double voxel;            /* edge length, > 0                                               */
  double trunc;            /* truncation distance, > 0 (typically 3..5 voxels)               */
  float  max_weight;       /* > 0: the weight saturates here, so the model can follow change */
} pm_tsdf_volume;
typedef struct pm_tsdf_integrate_options { float min_disp; float max_range; } pm_tsdf_integrate_options;
typedef struct pm_tsdf_raycast_options {
  float min_range, max_range;
  float step;              /* fraction of trunc, in (0, 1]                                   */
  float min_weight;        /* a voxel takes part iff weight > 0 and >= min_weight            */
} pm_tsdf_raycast_options;

size_t pm_tsdf_bytes(const pm_tsdf_volume* volume);   /* 0 if invalid or too large */
int pm_tsdf_clear(pm_handle* h, const pm_tsdf_volume* volume, void* d_voxels);
int pm_tsdf_integrate(pm_handle* h, const pm_cloud_camera* camera, const pm_tsdf_volume* volume,
                      const pm_motion* pose /* X_cam = R X_world + t */, const pm_tsdf_integrate_options* options,
                      const float* d_disp, const float* d_weight /* may be NULL */, int rows, int cols, void* d_voxels,
                      int* d_counts /* device int[2]: voxels in view, voxels updated; may be NULL */,
                      int* counts /* host int[2], may be NULL: non-NULL synchronises like pm_point_cloud's count */);
int pm_tsdf_raycast(pm_handle* h, const pm_cloud_camera* camera, const pm_tsdf_volume* volume, const pm_motion* pose,
                    const pm_tsdf_raycast_options* options, const void* d_voxels, int rows, int cols,
                    float* d_disp_out /* may be NULL */, float* d_normals_out /* [rows][cols][3], may be NULL */,
                    int* d_counts /* device int[1]: pixels hit; may be NULL */,
                    int* counts /* host int[1], may be NULL: non-NULL synchronises */);

/* ---- the model taken out of the volume: its zero level set as ONE welded triangle mesh in the world frame ------------------------
 * pm_tsdf_raycast followed by pm_grid_mesh gives what one pose sees, in that camera's frame.  pm_tsdf_mesh gives the whole surface
 * the volume holds: an indexed mesh with one vertex per crossed grid edge, shared by every triangle around it, compacted in a fixed
 * order.  The method is marching tetrahedra over the Kuhn (Freudenthal) split of every cell into six tetrahedra around the
 * diagonal 000-111 -- the same split in every cell, so faces match between neighbours, the mesh is closed wherever the observed
 * volume is, and there are no ambiguous cases.
 * Held to its CPU definition (tests/tsdf_mesh_ref.py) BIT FOR BIT; one rounding per operation, parentheses as written:
 *   observed  node (i, j, k) is OBSERVED iff weight > 0, weight >= min_weight and tsdf is finite; an observed node is INSIDE iff
 *             not (tsdf > 0): pm_tsdf_raycast's front crossing.
 *   cell      (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, is LIVE iff its eight corner nodes are observed; only live cells emit
 *             triangles.
 *   edges     node a owns seven edges a -> a + d, d = (1,0,0), (0,1,0), (0,0,1), (1,1,0), (0,1,1), (1,0,1), (1,1,1) in this
 *             order.  An edge CROSSES iff both ends are observed and exactly one is inside; it is a VERTEX iff it crosses and lies
 *             in at least one live cell, so every vertex is named by a triangle.
 *   vertex    t = (double)f_a / ((double)f_a - (double)f_b), a the owning node;  P_c = origin[c] + (((double)a_c + (d_c ? t : 0.0))
 *             * voxel);  xyz_c = (float)P_c.
 *   normal    G_c(n) = T(n + e_c) - T(n - e_c) in binary32, valid iff the six neighbours of n lie inside the grid and are observed;
 *             g_c = (double)Ga_c + (t * ((double)Gb_c - (double)Ga_c));  n_c = (float)g_c;  l = sqrtf(((n0*n0) + (n1*n1)) +
 *             (n2*n2));  (0, 0, 0) unless both gradients are valid and l > 0 and finite, else n_c / l.  World frame; it points to
 *             the positive side, which is free space.
 *   tetrahedra  for the axis orders p = xyz, xzy, yxz, yzx, zxy, zyx: c0 = 000, c1 = c0 + e_p0, c2 = c1 + e_p1, c3 = 111.  With I
 *             the inside corners and O the outside ones by corner number:  |I| = 1, I = {a}: the polygon is the edges (a, o), o
 *             ascending;  |I| = 3, O = {a}: (i, a), i ascending;  |I| = 2, I = {a < b}, O = {c < d}: (a, c), (a, d), (b, d), (b, c).
 *             With every polygon vertex at its edge's midpoint in doubled integer corner coordinates the polygon is read back to
 *             front iff ((Q1 - Q0) x (Q2 - Q0)) . (|I| sum(O) - |O| sum(I)) < 0.  Triangles (q0, q1, q2) and, of a quad,
 *             (q0, q2, q3): (P1 - P0) x (P2 - P0) points to the positive side, pm_grid_mesh's convention.  At most 12 per cell.
 *   order     vertices by owning node, x fastest, then by edge number; triangles by cell, x fastest, then by tetrahedron, then as
 *             above.  A triangle is three int32 vertex slots.
 *   counts    [vertices, triangles], whatever the capacities: exactly the first vertex_capacity vertices and the first
 *             tri_capacity triangles are written and nothing behind them; the indices always use the untruncated numbering
 *             (pm_grid_mesh's rules).  Every output is optional; capacities of 0 only count.
 * An inside node with tsdf == 0 makes its vertices coincide at the node: the ZERO-AREA triangles are emitted, because the topology
 * stays closed.  A grid thinner than two nodes on any axis is legal and empty.
 * Runs on the handle's stream, valid in every mode; a non-NULL host `counts` synchronises.  Seven launches at the most, the order
 * from arithmetic and never from an atomic, so two calls give the same bytes.  Scratch: 5 bytes per node, 8 per 64-node span of
 * a row and 8 per 1024 spans, ONE handle-owned allocation made on first use, reused, released with the handle; GROWING it
 * synchronises the stream, as pm_grid_mesh's does.
 * PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued: a null volume, options or d_voxels; a volume
 * pm_tsdf_integrate refuses; a min_weight that is NaN or < 0; a negative capacity.  PM_ERR_SIZE: nx * ny * nz > 2^31 - 1, or
 * 12 x cells or 7 x nodes above 2^31 - 1. */
typedef struct pm_tsdf_mesh_options { float min_weight; } pm_tsdf_mesh_options;
int pm_tsdf_mesh(pm_handle* h, const pm_tsdf_volume* volume, const pm_tsdf_mesh_options* options, const void* d_voxels,
                 int vertex_capacity, int tri_capacity, float* d_xyz_out /* [vertex_capacity][3], may be NULL */,
                 float* d_normals_out /* [vertex_capacity][3], may be NULL */,
                 int32_t* d_tri_out /* [tri_capacity][3], may be NULL */,
                 int* d_counts /* device int[2]: vertices, triangles; may be NULL */,
                 int* counts /* host int[2], may be NULL: non-NULL synchronises */);

/* ---- dense frame-to-model alignment: the pose of a new map against a render of the model, or against an earlier map ------------
 * What it is for: pm_tsdf_integrate folds a map into the model at its pose and pm_tsdf_raycast renders the model at any pose; the
 * pose has to come from somewhere.  pm_estimate_motion tracks sparse texture between two consecutive frames, and chained frame to
 * frame its errors add up.  pm_align_disparity registers the NEW frame's disparity map against the MODEL's map and camera-facing
 * normals (pm_tsdf_raycast's outputs, or any earlier map with pm_disparity_normals / pm_planes_normals): point-to-plane
 * Gauss-Newton with projective association, every pixel a residual, no texture needed.  The motion goes from the MODEL camera frame
 * into the NEW camera frame, X_new = R X_model + t -- pm_reproject_disparity's convention, so the result goes to that stage
 * unchanged; the pose of a frame aligned against a render at pose_ref is pm_motion_compose(M, pose_ref).
 * Held to its CPU definition (tests/align_ref.py) BIT FOR BIT.  Binary64 unless it says binary32, one rounding per operation,
 * parentheses as written; fxB = fx * baseline formed once.  Per model pixel (x, y), independent of every other pixel:
 *   model     d = Dm(y, x) counts iff d > 0 && d >= min_disp; n = Nm(y, x, :) counts iff its three components are finite and not
 *             all zero; P = pm_reproject_disparity's point of (d, x, y).  Otherwise the class is NO_MODEL (0).
 *   project   EXACTLY pm_reproject_disparity's `splat` arithmetic from its motion line on, with max_disp = 0: Q = (Xn, Yn, Zn),
 *             dq = (float)(fxB / Zn), (iu, iv).  A dropped pixel has class OUTSIDE (1).
 *   measure   d2 = Dn(iv, iu) counts iff d2 > 0 && d2 >= min_disp; otherwise UNMEASURED (2).
 *   gate      fabs((double)dq - (double)d2) <= (double)max_diff; otherwise GATED (3): occlusions and what came into view.
 *   point     P2 = the point of (d2, iu, iv), in the new frame.
 *   normal    m_i = ((R[3i]*(double)n0) + (R[3i+1]*(double)n1)) + (R[3i+2]*(double)n2).
 *   residual  e = ((m0*(Qx-P2x)) + (m1*(Qy-P2y))) + (m2*(Qz-P2z)), metres;  s = (P2z*P2z) / fxB, the metres per pixel of
 *             disparity at the measurement (stereo depth noise grows with Z^2);  r = e / s, pixels of disparity.
 *   row       a0 = (P2y*m2) - (P2z*m1); a1 = (P2z*m0) - (P2x*m2); a2 = (P2x*m1) - (P2y*m0);  J = (a0, a1, a2, m0, m1, m2), each
 *             / s: the derivative of r under pm_solve_motion's left perturbation Q' = Q + omega x Q + upsilon, the normal turning
 *             with it; delta = (omega, upsilon).
 *   weight    ar = fabs(r); w = 1.0 if ar <= huber_px, else huber_px / ar.
 *   terms     28: H_jk = (w*J_j)*J_k for j <= k, row-major upper triangle (21); g_j = (w*J_j)*r (6); r*r (1).  The class is
 *             USED (4).  A pixel of any other class contributes +0.0 to all 28.
 *   planes    d_class_out: the class; d_residual_out: (float)r for USED, +0.0f elsewhere.
 * The sum -- its order is part of the definition, binary64 addition not being associative.  With C = ceil(cols / 64): lane sums
 * A[y][l] = sum over c ascending from +0.0 of term(y, 64c + l), pixels at or beyond cols being +0.0; the row sum is the balanced
 * binary tree over l, s[i] = s[2i] + s[2i+1] six times; the total adds the row sums in ascending y from +0.0.  Counts: the model
 * pixels (class != NO_MODEL), the pixels that reached the gate (GATED + USED) and the USED pixels.
 * The solve is pm_solve_motion's, shared with it: H delta = -g by LDL^T without pivoting, which fails iff a pivot is not > 0; the
 * Cayley update; it stops after the update when max |delta_i| < epsilon, or after `iterations` updates.  One more evaluation under
 * the motion reached gives the counts, rms_px = sqrt(sum_rr / n_used) (0 without a used pixel) and the 21 entries of H -- the
 * information matrix a caller's pose filter wants.  valid iff no factorisation failed and n_used >= min_used; otherwise the call
 * returns PM_OK with info->valid == 0 and *out equal to the guess (pm_solve_motion's rule: no new status code).
 * pm_align_evaluate: one evaluation under `motion`; it only enqueues on the handle's stream (a non-NULL host `sums`
 * synchronises) and is valid in every mode.  Two launches behind a 16-byte memset; no atomics on floating-point values and no
 * cross-workgroup waits, so the record is a pure function of the inputs.  pm_align_step (host, no handle): one solve and update
 * from a record; where the factorisation fails it returns PM_OK with *out = *in, delta all +0.0 and *factorised = 0.
 * pm_align_disparity loops the two and always synchronises.  pm_motion_compose (host, no handle): X -> a(b(X)),
 * R_ij = ((a_i0*b_0j) + (a_i1*b_1j)) + (a_i2*b_2j); t_i = (((a_i0*bt0) + (a_i1*bt1)) + (a_i2*bt2)) + at_i; out may alias a or b.
 * Scratch: `rows` row sums of 28 doubles behind a 256-byte slot for the record, ONE handle-owned allocation made on first use, reused, grown
 * under a stream synchronisation and released with the handle, and one record of page-locked host memory for the downloads.
 * PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued: a null required pointer; a camera pm_backproject
 * refuses; a non-finite entry of the motion; options outside their ranges below, NaN included (min_disp: NaN); rows or cols < 1;
 * no output at all.  PM_ERR_SIZE as for pm_backproject.  The host-only calls report a refusal by their status alone. */
enum { PM_ALIGN_NO_MODEL = 0, PM_ALIGN_OUTSIDE = 1, PM_ALIGN_UNMEASURED = 2, PM_ALIGN_GATED = 3, PM_ALIGN_USED = 4 };
typedef struct pm_align_options {
  float min_disp;
  float max_diff;     /* >= 0, finite: the gate, in pixels of disparity */
  double huber_px;    /* > 0 */
  int iterations;     /* 1..50 */
  double epsilon;     /* >= 0 */
  int min_used;       /* >= 6 */
} pm_align_options;
typedef struct pm_align_sums {   /* 240 bytes */
  double H[21], g[6], rr;
  int n_model, n_gate, n_used, pad;
} pm_align_sums;
typedef struct pm_align_info {
  int valid, n_model, n_gate, n_used, iterations;
  double rms_px;
  double H[21];
} pm_align_info;

int pm_align_evaluate(pm_handle* h, const pm_cloud_camera* camera, const pm_align_options* options,
                      const pm_motion* motion /* NULL = identity */, const float* d_disp_model,
                      const float* d_normals_model /* [rows][cols][3] */, const float* d_disp_new, int rows, int cols,
                      uint8_t* d_class_out /* may be NULL */, float* d_residual_out /* may be NULL */,
                      pm_align_sums* d_sums /* device, may be NULL */,
                      pm_align_sums* sums /* host, may be NULL: non-NULL synchronises */);
int pm_align_step(const pm_align_sums* sums, const pm_motion* in /* NULL = identity */, pm_motion* out,
                  double delta[6] /* may be NULL */, int* factorised /* may be NULL */);   /* host only, no handle */
int pm_align_disparity(pm_handle* h, const pm_cloud_camera* camera, const pm_align_options* options,
                       const pm_motion* guess /* NULL = identity */, const float* d_disp_model, const float* d_normals_model,
                       const float* d_disp_new, int rows, int cols, pm_motion* out /* may be NULL */,
                       pm_align_info* info /* may be NULL */);
int pm_motion_compose(const pm_motion* a, const pm_motion* b, pm_motion* out);           /* host only, no handle */

/* ---- colour in the model: a colour volume beside the distance volume, integrated with it and gathered back -----------------------
 * The distance volume keeps a running weighted mean of the projective distance; the colour volume keeps the same mean of the
 * colour each frame saw at the surface, so the noisy, view-dependent colour of the frames is fused, not thrown away.  The colour
 * volume is caller-owned like the distance volume: nx * ny * nz records of 16 bytes {float b, g, r, weight}, x fastest, 16-byte
 * aligned (pm_device_malloc gives that); weight == 0: never coloured.  pm_tsdf_integrate_color does what pm_tsdf_integrate does and
 * colours; pm_tsdf_color_map reads the colour back at the pixels of any left map at a pose (a render of the model, or the measured
 * map itself), pm_tsdf_color_points at any world-frame points (pm_tsdf_mesh's vertices).
 * Held to its CPU definition (tests/tsdf_color_ref.py) BIT FOR BIT.  Binary64 unless it says binary32, one rounding per operation,
 * parentheses as written.
 *   integrate, per voxel:
 *     distance  everything pm_tsdf_integrate does, with its arithmetic (one shared statement): point, project, measure, weight,
 *               update.  The distance volume behind this call is BIT-IDENTICAL to what pm_tsdf_integrate writes from the same
 *               arguments, and so are counts [0] and [1].
 *     band      bandw = (double)band * trunc, formed once on the host.  A voxel that was updated is COLOURED iff sdf <= bandw and
 *               sdf >= -bandw and, with d_bgr, the three floats of pixel (iv, iu) are finite.
 *     pixel     the one the disparity came from: p_c = (float)bgr8[iv][iu][c], or bgr[iv][iu][c] as it is; c = 0, 1, 2 = b, g, r.
 *     update    binary32, w the colour record's own weight, wn the observation's weight (1.0f, or W(iv, iu)):
 *               C'_c = ((C_c * w) + (p_c * wn)) / (w + wn);  w' = fminf(w + wn, max_weight).
 *               A voxel that is not coloured keeps its 16 bytes and is neither read nor written.
 *     counts    [0] voxels in view, [1] voxels updated, [2] voxels coloured.
 *   sample at grid coordinates q (both gathers):
 *     guard     dropped unless fabs(q_i) < 2^30 on every axis (NaN and +-inf fail).
 *     cell      lo_i = floor(q_i);  fr_i = (float)(q_i - lo_i).
 *     corners   c = 0..7, bit 0 x, bit 1 y, bit 2 z, at lo + bits;  binary32 tw = (wx * wy) * wz with w = 1.0f - fr on a 0 bit and
 *               fr on a 1 bit.  A corner TAKES PART iff it lies inside the grid, its weight is > 0 and >= min_weight and its three
 *               channels are finite.  A corner outside the grid is never read, and there is no inside test on the point itself: a
 *               vertex on the grid's last node plane, a position a hair outside the grid and a grid one node thick all work.
 *     mean      binary32, from +0.0f, in ascending corner order, corners that take no part skipped:  den = den + tw;
 *               num_c = num_c + (tw * C_c).  COLOURED iff den > 0, and then value_c = num_c / den: a NORMALISED trilinear mean (the
 *               band is thin, corners behind the surface often hold no colour).
 *     outputs   d_bgr_out: value_c;  d_bgr8_out: (uint8)fminf(fmaxf(rintf(value_c * byte_scale), 0), 255), rintf half to even and
 *               fmaxf / fminf returning the other operand for a NaN;  zeros in both where not coloured.  counts [0] coloured.
 *   pm_tsdf_color_map, per pixel (x, y):  d = D(y, x) counts iff d > 0 (never NaN);  s = fxB / (double)d;  the grid coordinates are
 *     pm_tsdf_raycast's own: its inverse pose, dx, dy, wd_i and q_i = ((c_i + (s * wd_i)) - origin[i]) / voxel.
 *   pm_tsdf_color_points, per point:  q_i = ((double)P_i - origin[i]) / voxel.  With d_n only the first min(n, *d_n) points are
 *     worked on (a *d_n < 0 counts as 0); the outputs of the others keep their bytes.  d_n is read on the device, behind whatever the
 *     stream ran before: pm_tsdf_mesh's device vertex count goes in directly.
 * All calls enqueue on the handle's stream and are valid in every mode of the handle; a non-NULL host `counts` synchronises, as
 * pm_tsdf_integrate's does.  pm_tsdf_color_clear is one memset ({+0.0f} x 4); the others are one launch behind a 16-byte memset.  No
 * voxel, pixel or point is touched by two threads and only integer addition crosses workgroups.  Scratch is the 16 bytes of the
 * counts that pm_tsdf_integrate and pm_tsdf_raycast already share: handle-owned, allocated on first use, released with the handle.
 * PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued, the checks in this order -- integrate:
 * whatever pm_tsdf_integrate refuses, in its order; a null d_colors; both or neither of d_bgr8 and d_bgr; a band that is NaN or
 * outside (0, 1].  map: a camera pm_backproject refuses; a null volume, pose, options or d_colors; a volume pm_tsdf_integrate
 * refuses; a non-finite entry of the pose; a null d_disp; a min_weight that is NaN or < 0; a byte_scale that is not finite or
 * not > 0; rows or cols < 1; no output at all (d_bgr_out, d_bgr8_out, d_counts and counts all NULL).  points: a null volume,
 * options, d_colors or d_xyz (n == 0 included); the volume; min_weight; byte_scale; n < 0; no output at all.  n == 0 is legal and
 * only zeroes the count.  PM_ERR_SIZE: nx * ny * nz > 2^31 - 1; more pixels than pm_backproject takes; n > (2^31 - 1) / 3. */
typedef struct pm_tsdf_color_options {   /* integrate */
  float min_disp, max_range;             /* pm_tsdf_integrate_options' two, same rules          */
  float band;                            /* in (0, 1]: colour is taken iff |sdf| <= band * trunc */
} pm_tsdf_color_options;
typedef struct pm_tsdf_color_sample_options {
  float min_weight;                      /* a corner takes part iff weight > 0 and >= min_weight */
  float byte_scale;                      /* finite, > 0: bytes = saturate(rintf(value * byte_scale)) */
} pm_tsdf_color_sample_options;

size_t pm_tsdf_color_bytes(const pm_tsdf_volume* volume);   /* 16 per voxel; 0 where pm_tsdf_bytes is 0 */
int pm_tsdf_color_clear(pm_handle* h, const pm_tsdf_volume* volume, void* d_colors);
int pm_tsdf_integrate_color(pm_handle* h, const pm_cloud_camera* camera, const pm_tsdf_volume* volume,
                            const pm_motion* pose /* X_cam = R X_world + t */, const pm_tsdf_color_options* options,
                            const float* d_disp, const float* d_weight /* may be NULL */,
                            const uint8_t* d_bgr8 /* [rows][cols][3] */, const float* d_bgr /* [rows][cols][3] */,
                            /* exactly one of the two */
                            int rows, int cols, void* d_voxels, void* d_colors,
                            int* d_counts /* device int[3]: in view, updated, coloured; may be NULL */,
                            int* counts /* host int[3], may be NULL: non-NULL synchronises */);
int pm_tsdf_color_map(pm_handle* h, const pm_cloud_camera* camera, const pm_tsdf_volume* volume, const pm_motion* pose,
                      const pm_tsdf_color_sample_options* options, const void* d_colors, const float* d_disp, int rows, int cols,
                      float* d_bgr_out /* [rows][cols][3], may be NULL */, uint8_t* d_bgr8_out /* [rows][cols][3], may be NULL */,
                      int* d_counts /* device int[1]: coloured; may be NULL */,
                      int* counts /* host int[1], may be NULL: non-NULL synchronises */);
int pm_tsdf_color_points(pm_handle* h, const pm_tsdf_volume* volume, const pm_tsdf_color_sample_options* options,
                         const void* d_colors, const float* d_xyz /* [n][3], world frame */, int n,
                         const int* d_n /* device, may be NULL: only the first min(n, *d_n) */,
                         float* d_bgr_out /* [n][3], may be NULL */, uint8_t* d_bgr8_out /* [n][3], may be NULL */,
                         int* d_counts /* device int[1]: coloured; may be NULL */,
                         int* counts /* host int[1], may be NULL: non-NULL synchronises */);

/* ---- a photometric term for the dense alignment: the model's colour against the new image --------------------------------------
 * pm_align_disparity is point-to-plane only: on a fronto-parallel plane -- a camera looking down at a flat seabed -- three of the
 * six parameters are free.  pm_tsdf_color_map renders the model's colour beside pm_tsdf_raycast's map and normals; the term below
 * compares it with the new image where each model pixel projects to, and pm_align_color_disparity runs pm_align_disparity's loop
 * on the sum of both terms.  Held to its CPU definition (tests/align_photo_ref.py) BIT FOR BIT.  Binary64 unless it says binary32,
 * one rounding per operation, parentheses as written.  The motion, the classes, the 28 terms, the 240-byte record and the ORDER of
 * the sum are pm_align_evaluate's.
 *   pm_bgr_luma, per pixel, binary32: p_c = (float)byte, or the float as it is;  L = ((b * 0.114f) + (g * 0.587f)) + (r * 0.299f).
 *     The output is the quiet NaN 0x7FC00000 where a channel is not finite, or where zero_is_absent != 0 and all three channels
 *     are == 0 (pm_tsdf_color_map's "not coloured").  NaN is the one "absent" marker of a luma plane.  One launch.
 *   pm_align_photo_evaluate, per model pixel (x, y):
 *     model     d = Dm(y, x) counts as in pm_align_evaluate;  Lm = (double)Lum_m(y, x) counts iff finite.  Otherwise NO_MODEL.
 *               P = pm_reproject_disparity's point of (d, x, y).
 *     project   pm_align_evaluate's, untouched: Q = (Xn, Yn, Zn), dq, (iu, iv); a dropped pixel is OUTSIDE.  Then
 *               u = (fx * (Xn / Zn)) + cx;  v = (fy * (Yn / Zn)) + cy (that projection's own expressions, recomputed);
 *               x0 = floor(u); y0 = floor(v), in binary64;  OUTSIDE also unless x0 >= 0 && x0 + 1 <= cols - 1 && y0 >= 0 &&
 *               y0 + 1 <= rows - 1: an image of one column or one row has no USED pixel.
 *     measure   d2 = Dn(iv, iu) counts as d does;  the taps L00 = Ln(y0, x0), L01 = Ln(y0, x0 + 1), L10 = Ln(y0 + 1, x0),
 *               L11 = Ln(y0 + 1, x0 + 1) are all finite.  Otherwise UNMEASURED.  d2 is read first, the taps only where it counts.
 *     gate      fabs((double)dq - (double)d2) <= (double)max_diff; otherwise GATED: the geometric term's occlusion test.
 *     sample    the taps converted to binary64;  a = u - x0;  b = v - y0;  dt = L01 - L00;  db = L11 - L10;
 *               top = L00 + (a * dt);  bot = L10 + (a * db);  val = top + (b * (bot - top));  gx = dt + (b * (db - dt));
 *               gy = bot - top: the bilinear value and the exact gradient of the bilinear interpolant, from four taps.
 *     residual  r = val - Lm, in levels.
 *     row       bx = (gx * fx) / Qz;  by = (gy * fy) / Qz;  bz = -(((bx * Qx) + (by * Qy)) / Qz);
 *               J = ((Qy*bz) - (Qz*by), (Qz*bx) - (Qx*bz), (Qx*by) - (Qy*bx), bx, by, bz): the derivative of r under the same left
 *               perturbation Q' = Q + omega x Q + upsilon, so pm_align_step solves it unchanged.
 *     weight    ar = fabs(r); w = 1.0 if ar <= huber_levels, else huber_levels / ar.
 *     terms, sum, counts, planes: pm_align_evaluate's, r in levels.
 *   pm_align_sums_blend (host, no handle): l2 = lambda * lambda, formed once; each of the 28 doubles is geo + (l2 * photo); the
 *     three counts are integer sums, pad is 0; out may alias either input.  lambda converts levels into pixels of disparity
 *     (sigma_d / sigma_I).  PM_ERR_INVALID_ARG by status alone: a null pointer; a lambda that is not finite or < 0.
 *   pm_align_color_disparity: the two luma planes once per call (the model's with zero_is_absent = 1, the new image's with 0);
 *     per update one pm_align_evaluate and one pm_align_photo_evaluate under the same motion (the photometric term with align's
 *     min_disp and max_diff), both records behind ONE synchronisation, pm_align_sums_blend, pm_align_step.  The stop rule and the
 *     "invalid answer is the guess" rule are pm_align_disparity's.  One more pair of evaluations under the motion reached gives
 *     the info: geo as pm_align_disparity fills it from the geometric record (geo.valid the call's validity, geo.iterations its
 *     updates, geo.H the geometric matrix), the photometric counts, rms_levels = sqrt(rr_photo / n_photo_used) (0 without a used
 *     pixel) and H, the blended matrix.  valid iff no factorisation failed and geo.n_used + n_photo_used >= align.min_used.
 * The device calls enqueue on the handle's stream and are valid in every mode; a non-NULL host `sums` synchronises, and
 * pm_align_color_disparity always does.  An evaluation is two launches behind a 16-byte memset (its second launch is
 * pm_align_evaluate's); no atomics on floating-point values, no cross-workgroup waits: two runs give the same bytes.
 * Scratch: a second 256-byte record slot and a second run of `rows` row sums, then the loop's two luma planes, in ONE further
 * handle-owned allocation (256 + 224 rows + 8 rows cols bytes) made on first use, grown under a stream synchronisation and
 * released with the handle, and one further page-locked record.  pm_align_evaluate's own scratch is as it was.
 * PM_ERR_INVALID_ARG, with pm_last_error naming the argument and nothing enqueued, the checks in this order -- luma: both or
 * neither of d_bgr8 and d_bgr; a null d_luma_out; rows or cols < 1.  evaluate: a camera pm_backproject refuses; a null options,
 * d_disp_model, d_luma_model, d_disp_new or d_luma_new; a non-finite entry of the motion; min_disp NaN; max_diff not finite or
 * < 0; huber_levels not > 0; rows or cols < 1; no output at all.  loop: whatever pm_align_disparity refuses, in its order; a null
 * d_bgr_model; both or neither of d_bgr8_new and d_bgr_new; huber_levels; a lambda that is not finite or < 0.  PM_ERR_SIZE as for
 * pm_backproject. */
typedef struct pm_align_photo_options {
  float min_disp;
  float max_diff;        /* >= 0, finite: the gate, in pixels of disparity */
  double huber_levels;   /* > 0 */
} pm_align_photo_options;
typedef struct pm_align_color_options {
  pm_align_options align;   /* the geometric term and the loop */
  double huber_levels;      /* > 0 */
  double lambda;            /* finite, >= 0: levels into pixels of disparity */
} pm_align_color_options;
typedef struct pm_align_color_info {
  pm_align_info geo;
  int n_photo_model, n_photo_gate, n_photo_used;
  double rms_levels;
  double H[21];             /* the blended matrix */
} pm_align_color_info;

int pm_bgr_luma(pm_handle* h, const uint8_t* d_bgr8 /* [rows][cols][3] */, const float* d_bgr /* [rows][cols][3] */,
                /* exactly one of the two */
                int rows, int cols, int zero_is_absent, float* d_luma_out /* [rows][cols] */);
int pm_align_photo_evaluate(pm_handle* h, const pm_cloud_camera* camera, const pm_align_photo_options* options,
                            const pm_motion* motion /* NULL = identity */, const float* d_disp_model,
                            const float* d_luma_model, const float* d_disp_new, const float* d_luma_new, int rows, int cols,
                            uint8_t* d_class_out /* may be NULL */, float* d_residual_out /* may be NULL */,
                            pm_align_sums* d_sums /* device, may be NULL */,
                            pm_align_sums* sums /* host, may be NULL: non-NULL synchronises */);
int pm_align_sums_blend(const pm_align_sums* geo, const pm_align_sums* photo, double lambda,
                        pm_align_sums* out);                                              /* host only, no handle */
int pm_align_color_disparity(pm_handle* h, const pm_cloud_camera* camera, const pm_align_color_options* options,
                             const pm_motion* guess /* NULL = identity */, const float* d_disp_model,
                             const float* d_normals_model,
                             const float* d_bgr_model /* [rows][cols][3]: pm_tsdf_color_map's d_bgr_out */,
                             const float* d_disp_new, const uint8_t* d_bgr8_new, const float* d_bgr_new,
                             /* exactly one of the two */
                             int rows, int cols, pm_motion* out /* may be NULL */, pm_align_color_info* info /* may be NULL */);

/* ---- device buffers for host code that does not include HIP (host/imaging.hpp uses them) ------------------
 * pm_device_malloc / pm_device_free wrap hipMalloc / hipFree on the handle's device; pm_upload / pm_download are
 * stream-ordered copies on the handle's stream from / to pageable host memory (pm_download returns after the
 * data has arrived). */
int pm_device_malloc(pm_handle* h, size_t bytes, void** d_ptr);
int pm_device_free(pm_handle* h, void* d_ptr);
int pm_upload(pm_handle* h, void* d_dst, const void* src, size_t bytes);
int pm_download(pm_handle* h, void* dst, const void* d_src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
