// pm_align_photo_body.hpp -- the per-pixel arithmetic and the per-thread bodies of pm_bgr_luma and pm_align_photo_evaluate
// (include/pm/imaging.h), host-callable and free of kernels, so that the kernels (pm_align_photo.hpp) and a CPU build
// (tests/cpp/align_photo_host_main.cpp, under the sanitizers) share ONE statement of it.  The definition it is held to BIT FOR BIT
// is tests/align_photo_ref.py: every operation is one rounding in binary64 unless binary32 is named,
// parentheses as written (-ffp-contract=off).  The model pixel's point and its projection are pm_reproject_body.hpp's, the 28
// terms, the lane's tail, the tree and the total are pm_align_body.hpp's: only the residual and its row are new here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_align_body.hpp"

namespace pm {

constexpr unsigned kLumaAbsentBits = 0x7FC00000u;  // the one "absent" marker of a luma plane: this quiet NaN

// ---- pm_bgr_luma ------------------------------------------------------------------------------------------------------------
struct LumaArgs {
  const uint8_t* bgr8;  // [rows][cols][3], or null
  const float* bgr;     // [rows][cols][3], or null: exactly one of the two
  int rows, cols;
  int zero_is_absent;
  float* luma;  // [rows][cols]
};

// The blocks of k_bgr_luma: (64, 4) threads, one pixel per lane.
struct LumaBlocks {
  unsigned x, y;
};
inline LumaBlocks luma_blocks(int rows, int cols) {
  return LumaBlocks{(unsigned)((cols + kAlignBlockX - 1) / kAlignBlockX), (unsigned)((rows + kAlignBlockY - 1) / kAlignBlockY)};
}

__host__ __device__ __forceinline__ float bgr_luma(float b, float g, float r, bool zero_is_absent) {
  const bool finite = b - b == 0.f && g - g == 0.f && r - r == 0.f;  // false for NaN and for +-inf
  const bool absent = !finite || (zero_is_absent && b == 0.f && g == 0.f && r == 0.f);
  const float L = ((b * 0.114f) + (g * 0.587f)) + (r * 0.299f);
  return absent ? __builtin_bit_cast(float, kLumaAbsentBits) : L;
}

// The work of one thread of k_bgr_luma: pixel (x, y) inside the image.
__host__ __device__ __forceinline__ void luma_lane(const LumaArgs& a, int x, int y) {
  const size_t px = (size_t)y * a.cols + x;
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = a.bgr8 ? (float)a.bgr8[px * 3 + k] : a.bgr[px * 3 + k];
  a.luma[px] = bgr_luma(c[0], c[1], c[2], a.zero_is_absent != 0);
}

// ---- pm_align_photo_evaluate -------------------------------------------------------------------------------------------------
// The launch's one argument, by value, as AlignArgs: wave-uniform, in scalar registers.
struct AlignPhotoArgs {
  CloudCam cam;
  double R[9], t[3];  // X_new = R X_model + t
  float min_disp, max_diff;
  double huber_levels;
  const float* disp_model;  // [rows][cols]
  const float* luma_model;  // [rows][cols]
  const float* disp_new;    // [rows][cols]
  const float* luma_new;    // [rows][cols]
  int rows, cols;
  uint8_t* class_out;   // [rows][cols]; may be null
  float* residual_out;  // [rows][cols]; may be null
  double* row_sums;     // [rows][kAlignTerms]
  int* counts;          // [0] model pixels, [1] pixels that reached the gate, [2] used pixels; zeroed
};

__host__ __device__ __forceinline__ bool luma_finite(float v) { return v - v == 0.f; }

// Model pixel (x, y) with disparity d and luma lm: its class and, where that is kAlignUsed, its 28 terms and its residual in
// levels.  The new map and then the four taps are read behind every earlier test: a pixel that fails early loads nothing more.
__host__ __device__ __forceinline__ int align_photo_pixel(const AlignPhotoArgs& a, int x, int y, float d, float lm,
                                                          double term[kAlignTerms], double* residual) {
  double P[3];
  const bool has_d = reproject_point(a.cam, a.min_disp, d, x, y, P);
  if (!(has_d && luma_finite(lm))) return kAlignNoModel;
  int iu, iv;
  float dq;
  double Q[3];
  if (!reproject_project(a.cam, a.R, a.t, 0.f, a.rows, a.cols, true, P, &iu, &iv, &dq, &Q[2], &Q[0], &Q[1])) return kAlignOutside;
  const double u = (a.cam.fx * (Q[0] / Q[2])) + a.cam.cx;  // reproject_project's own expressions: |u|, |v| < 2^30 behind it
  const double v = (a.cam.fy * (Q[1] / Q[2])) + a.cam.cy;
  const double x0f = __builtin_floor(u), y0f = __builtin_floor(v);
  if (!(x0f >= 0.0 && x0f + 1.0 <= (double)(a.cols - 1) && y0f >= 0.0 && y0f + 1.0 <= (double)(a.rows - 1))) return kAlignOutside;
  const float d2 = a.disp_new[(size_t)iv * a.cols + iu];
  if (!(d2 > 0.f && d2 >= a.min_disp)) return kAlignUnmeasured;
  const float* tap = a.luma_new + ((size_t)(int)y0f * a.cols + (int)x0f);  // the cell lies inside the image
  const float t00 = tap[0], t01 = tap[1], t10 = tap[a.cols], t11 = tap[a.cols + 1];
  if (!(luma_finite(t00) && luma_finite(t01) && luma_finite(t10) && luma_finite(t11))) return kAlignUnmeasured;
  if (!(__builtin_fabs((double)dq - (double)d2) <= (double)a.max_diff)) return kAlignGated;
  const double L00 = (double)t00, L01 = (double)t01, L10 = (double)t10, L11 = (double)t11;
  const double fa = u - x0f, fb = v - y0f;
  const double dt = L01 - L00, db = L11 - L10;
  const double top = L00 + (fa * dt), bot = L10 + (fa * db);
  const double val = top + (fb * (bot - top));
  const double gx = dt + (fb * (db - dt));
  const double gy = bot - top;
  const double r = val - (double)lm;
  const double bx = (gx * a.cam.fx) / Q[2];
  const double by = (gy * a.cam.fy) / Q[2];
  const double bz = -(((bx * Q[0]) + (by * Q[1])) / Q[2]);
  const double J[6] = {(Q[1] * bz) - (Q[2] * by), (Q[2] * bx) - (Q[0] * bz), (Q[0] * by) - (Q[1] * bx), bx, by, bz};
  align_terms(J, r, a.huber_levels, term);
  *residual = r;
  return kAlignUsed;
}

// One trip of one lane of k_align_photo_rows: pixel (x, y) inside the image, as align_lane.
__host__ __device__ __forceinline__ int align_photo_lane(const AlignPhotoArgs& a, int x, int y, double acc[kAlignTerms]) {
  const size_t px = (size_t)y * a.cols + x;
  const float d = a.disp_model[px];
  const float lm = a.luma_model[px];
  double term[kAlignTerms], r = 0.0;
  const int cls = align_photo_pixel(a, x, y, d, lm, term, &r);
  align_lane_tail(cls, term, r, px, a.class_out, a.residual_out, acc);
  return cls;
}

}  // namespace pm
