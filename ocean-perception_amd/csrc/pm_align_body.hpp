// pm_align_body.hpp -- the per-pixel arithmetic and the per-thread bodies of pm_align_evaluate (include/pm/imaging.h),
// host-callable and free of kernels, so that the kernels (pm_align.hpp) and a CPU build (tests/cpp/align_host_main.cpp, under
// the sanitizers) share ONE statement of it.  The definition it is held to BIT FOR BIT is tests/align_ref.py (DESIGN.md section
// 8c-12): every operation is one rounding in binary64 unless binary32 is named, parentheses as written (the build uses
// -ffp-contract=off; binary64 division and rint are IEEE on gfx950).  Carrying a model pixel into the new frame is
// pm_reproject_body.hpp's reproject_point and reproject_project, untouched.
// The ORDER of the sum is part of the definition: a lane adds the pixels x = 64 c + l of its row in ascending c from +0.0, the 64
// lane sums of a row meet in the balanced binary tree s[i] = s[2i] + s[2i+1] (align_tree here; the kernel's DPP sequence is the
// same tree), and the rows are added in ascending y.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_reproject_body.hpp"

namespace pm {

constexpr int kAlignLanes = 64;   // k_align_rows: a wavefront owns a row, lane l its pixels 64 c + l
constexpr int kAlignWaves = 4;    // rows per block
constexpr int kAlignBlockX = kAlignLanes;
constexpr int kAlignBlockY = kAlignWaves;
constexpr int kAlignTerms = 28;   // H's upper triangle row-major (21), g (6), r r (1): pm_align_sums' doubles in this order
constexpr int kAlignFinishBatch = 8;  // k_align_finish: row sums in flight per lane

enum : int { kAlignNoModel = 0, kAlignOutside = 1, kAlignUnmeasured = 2, kAlignGated = 3, kAlignUsed = 4 };

// The blocks of k_align_rows: one per kAlignBlockY rows.
inline unsigned align_row_blocks(int rows) { return (unsigned)((rows + kAlignBlockY - 1) / kAlignBlockY); }
// The chunks of a row: every lane of a wavefront makes this many trips.
__host__ __device__ __forceinline__ int align_chunks(int cols) { return (cols + kAlignLanes - 1) / kAlignLanes; }

// The launch's one argument, by value: the camera, the motion and the options are wave-uniform and stay in scalar registers.
struct AlignArgs {
  CloudCam cam;
  double R[9], t[3];  // X_new = R X_model + t
  float min_disp, max_diff;
  double huber_px;
  const float* disp_model;     // [rows][cols]
  const float* normals_model;  // [rows][cols][3]
  const float* disp_new;       // [rows][cols]
  int rows, cols;
  uint8_t* class_out;   // [rows][cols]; may be null
  float* residual_out;  // [rows][cols]; may be null
  double* row_sums;     // [rows][kAlignTerms]
  int* counts;          // [0] model pixels, [1] pixels that reached the gate, [2] used pixels; zeroed
};

// The 28 terms of a used pixel from its row J, its residual r and the Huber threshold in r's unit: shared by the geometric pixel
// below and the photometric one (pm_align_photo_body.hpp).
__host__ __device__ __forceinline__ void align_terms(const double J[6], double r, double huber, double term[kAlignTerms]) {
  const double ar = __builtin_fabs(r);
  const double w = ar <= huber ? 1.0 : huber / ar;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double wj = w * J[i];
#pragma unroll
    for (int j = i; j < 6; ++j) term[k++] = wj * J[j];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) term[21 + i] = (w * J[i]) * r;
  term[27] = r * r;
}

// The end of one trip of one lane: a pixel's terms are added to the lane's sums (a pixel that is not used adds +0.0 to each)
// and the optional planes are written.
__host__ __device__ __forceinline__ void align_lane_tail(int cls, const double term[kAlignTerms], double r, size_t px,
                                                         uint8_t* class_out, float* residual_out, double acc[kAlignTerms]) {
  const bool used = cls == kAlignUsed;
#pragma unroll
  for (int k = 0; k < kAlignTerms; ++k) acc[k] = acc[k] + (used ? term[k] : 0.0);
  if (class_out) class_out[px] = (uint8_t)cls;
  if (residual_out) residual_out[px] = used ? (float)r : 0.f;
}

// Model pixel (x, y) with disparity d and normal n: its class and, where that is kAlignUsed, its 28 terms and its residual in
// pixels of disparity.  The new map is read behind every earlier test.
__host__ __device__ __forceinline__ int align_pixel(const AlignArgs& a, int x, int y, float d, const float n[3],
                                                    double term[kAlignTerms], double* residual) {
  double P[3];
  const bool has_d = reproject_point(a.cam, a.min_disp, d, x, y, P);
  const bool finite = n[0] - n[0] == 0.f && n[1] - n[1] == 0.f && n[2] - n[2] == 0.f;  // false for NaN and for +-inf
  const bool has_n = finite && !(n[0] == 0.f && n[1] == 0.f && n[2] == 0.f);
  if (!(has_d && has_n)) return kAlignNoModel;
  int iu, iv;
  float dq;
  double Q[3];
  if (!reproject_project(a.cam, a.R, a.t, 0.f, a.rows, a.cols, true, P, &iu, &iv, &dq, &Q[2], &Q[0], &Q[1])) return kAlignOutside;
  const float d2 = a.disp_new[(size_t)iv * a.cols + iu];  // the one gather
  double P2[3];
  if (!reproject_point(a.cam, a.min_disp, d2, iu, iv, P2)) return kAlignUnmeasured;
  if (!(__builtin_fabs((double)dq - (double)d2) <= (double)a.max_diff)) return kAlignGated;
  const double n0 = (double)n[0], n1 = (double)n[1], n2 = (double)n[2];
  const double m0 = ((a.R[0] * n0) + (a.R[1] * n1)) + (a.R[2] * n2);
  const double m1 = ((a.R[3] * n0) + (a.R[4] * n1)) + (a.R[5] * n2);
  const double m2 = ((a.R[6] * n0) + (a.R[7] * n1)) + (a.R[8] * n2);
  const double e = ((m0 * (Q[0] - P2[0])) + (m1 * (Q[1] - P2[1]))) + (m2 * (Q[2] - P2[2]));
  const double s = (P2[2] * P2[2]) / a.cam.fxb;
  const double r = e / s;
  const double J[6] = {((P2[1] * m2) - (P2[2] * m1)) / s, ((P2[2] * m0) - (P2[0] * m2)) / s, ((P2[0] * m1) - (P2[1] * m0)) / s,
                       m0 / s, m1 / s, m2 / s};
  align_terms(J, r, a.huber_px, term);
  *residual = r;
  return kAlignUsed;
}

// One trip of one lane of k_align_rows: pixel (x, y) inside the image.  Its terms are added to the lane's sums (a pixel that is
// not used adds +0.0 to each), the optional planes are written, the class is returned.
__host__ __device__ __forceinline__ int align_lane(const AlignArgs& a, int x, int y, double acc[kAlignTerms]) {
  const size_t px = (size_t)y * a.cols + x;
  const float d = a.disp_model[px];
  const float* np = a.normals_model + px * 3;
  const float n[3] = {np[0], np[1], np[2]};
  double term[kAlignTerms], r = 0.0;
  const int cls = align_pixel(a, x, y, d, n, term, &r);
  align_lane_tail(cls, term, r, px, a.class_out, a.residual_out, acc);
  return cls;
}

// The row sum of one term: the balanced binary tree over the 64 lane sums, in place; the total is s[0].
__host__ __device__ __forceinline__ void align_tree(double s[kAlignLanes]) {
  for (int n = kAlignLanes / 2; n >= 1; n /= 2)
    for (int i = 0; i < n; ++i) s[i] = s[2 * i] + s[2 * i + 1];
}

// The work of lane e < kAlignTerms of k_align_finish: term e of every row, added in ascending y from +0.0.
__host__ __device__ __forceinline__ double align_total(const double* row_sums, int rows, int e) {
  double sum = 0.0;
  int y = 0;
  for (; y + kAlignFinishBatch <= rows; y += kAlignFinishBatch) {
    double v[kAlignFinishBatch];
#pragma unroll
    for (int k = 0; k < kAlignFinishBatch; ++k) v[k] = row_sums[(size_t)(y + k) * kAlignTerms + e];  // in flight together
#pragma unroll
    for (int k = 0; k < kAlignFinishBatch; ++k) sum = sum + v[k];
  }
  for (; y < rows; ++y) sum = sum + row_sums[(size_t)y * kAlignTerms + e];
  return sum;
}

}  // namespace pm
