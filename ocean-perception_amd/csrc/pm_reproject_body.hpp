// pm_reproject_body.hpp -- the per-pixel arithmetic and the per-thread bodies of pm_reproject_disparity
// (include/pm/imaging.h), host-callable and free of kernels, so that the kernels (pm_reproject.hpp) and a CPU build
// (tests/cpp/reproject_host_main.cpp, under the sanitizers) share ONE statement of it.  The definition it is held to BIT
// FOR BIT is tests/reproject_ref.py: every operation is one rounding in the format written,
// parentheses as written (the build uses -ffp-contract=off; binary64 division and rint are IEEE on gfx950).
// Only one operation differs between the two builds: "raise a word to the maximum" is an integer atomicMax on the device
// and a plain maximum on the host (reproject_raise).  The maps in flight hold the BITS of +0.0 or of a finite binary32 > 0,
// so unsigned order is float order and `word != 0` is `value > 0`.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_cloud_body.hpp"

namespace pm {

constexpr int kReprojectTileW = 64;     // k_reproject_finish: pixels of a tile along a row (one wavefront)
constexpr int kReprojectTileH = 16;     // ... and its rows (four per thread)
constexpr int kReprojectMaxRadius = 3;  // the widest halo
constexpr int kReprojectTilePitch = kReprojectTileW + 2 * kReprojectMaxRadius;
constexpr int kReprojectTileWords = kReprojectTilePitch * (kReprojectTileH + 2 * kReprojectMaxRadius);

__host__ __device__ __forceinline__ void reproject_raise(unsigned* word, unsigned bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(word, bits);  // no return value is used: a fire-and-forget integer maximum
#else
  if (*word < bits) *word = bits;
#endif
}

__host__ __device__ __forceinline__ void reproject_add(int* word, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(word, n);
#else
  *word += n;
#endif
}

constexpr int kReprojectLanes = 64;         // splat launches: a wavefront takes 64 consecutive pixels of a row at a time ...
constexpr int kReprojectPixelsPerLane = 4;  // ... four times, 64 pixels apart: 256 pixels of a row per wavefront
constexpr int kReprojectBlockX = 64;        // splat launches: one wavefront along a row (256 pixels) ...
constexpr int kReprojectBlockY = 4;         // ... and rows per block; the finish launch: 64 x 4 threads per 64 x 16 tile
constexpr int kReprojectSpan = kReprojectLanes * kReprojectPixelsPerLane;  // pixels of a row per splat block

// The grid of the row-span launches (the seeds' splats here, the consistency filter and the fusion, whose constants are aliases
// of these): a block takes kReprojectSpan pixels of a row and kReprojectBlockY rows.  The one statement of it, for the launches
// (pm_stages.hip: span_grid) and for a CPU build that walks them (tests/cpp/host_launch.hpp).
struct SpanBlocks {
  unsigned x, y;  // blocks along a row, blocks down the rows
};
inline SpanBlocks span_blocks(int rows, int cols) {
  return SpanBlocks{(unsigned)((cols + kReprojectSpan - 1) / kReprojectSpan), (unsigned)((rows + kReprojectBlockY - 1) / kReprojectBlockY)};
}

// ---- stage 1: the old left map into the new left view -----------------------------------------------------------------------
struct ReprojectArgs {
  CloudCam cam;
  double R[9], t[3];
  float min_disp, max_disp;
  const float* disp;
  int rows, cols;
  unsigned* splat;  // [rows][cols], zeroed
};

// The two halves of carrying a pixel through a motion, shared with pm_filter_consistency (pm_consistency_body.hpp), which
// keeps the first half's point across its sources.  First half: the point P = (X, Y, Z) of pixel (x, y) with disparity d in
// binary64 (pm_backproject's values before their rounding); false where the pixel takes no part.
__host__ __device__ __forceinline__ bool reproject_point(const CloudCam& c, float min_disp, float d, int x, int y, double P[3]) {
  const bool ok = d > 0.f && d >= min_disp;
  const double Z = c.fxb / (double)(ok ? d : 1.f);
  P[0] = (((double)x - c.cx) * Z) / c.fx;
  P[1] = (((double)y - c.cy) * Z) / c.fy;
  P[2] = Z;
  return ok;
}

// Second half: P through X_new = R X + t and into the rows x cols image of the same camera: the pixel it lands on and the
// disparity it has there.  `ok`: the first half's answer; false where the point is dropped, and (iu, iv) is then (0, 0).
// Where asked for (pm_fuse_disparity, pm_fuse_body.hpp), the depth Zn in the new frame in *zn; where asked for
// (pm_align_disparity, pm_align_body.hpp), the rest of the point in the new frame in *xn and *yn.
__host__ __device__ __forceinline__ bool reproject_project(const CloudCam& c, const double R[9], const double t[3],
                                                           float max_disp, int rows, int cols, bool ok, const double P[3],
                                                           int* iu, int* iv, float* dn, double* zn = nullptr,
                                                           double* xn = nullptr, double* yn = nullptr) {
  const double X = P[0], Y = P[1], Z = P[2];
  const double Xn = (((R[0] * X) + (R[1] * Y)) + (R[2] * Z)) + t[0];
  const double Yn = (((R[3] * X) + (R[4] * Y)) + (R[5] * Z)) + t[1];
  const double Zn = (((R[6] * X) + (R[7] * Y)) + (R[8] * Z)) + t[2];
  ok = ok && Zn > 0.0;
  const float v = (float)(c.fxb / Zn);
  ok = ok && v > 0.f && v < __builtin_inff() && (max_disp == 0.f || v <= max_disp);
  const double u = (c.fx * (Xn / Zn)) + c.cx;
  const double w = (c.fy * (Yn / Zn)) + c.cy;
  const double lim = 1073741824.0;  // 2^30: what follows fits an int
  ok = ok && __builtin_fabs(u) < lim && __builtin_fabs(w) < lim;
  const double ru = __builtin_rint(u), rw = __builtin_rint(w);  // half to even
  ok = ok && ru >= 0.0 && ru < (double)cols && rw >= 0.0 && rw < (double)rows;
  *iu = ok ? (int)ru : 0;
  *iv = ok ? (int)rw : 0;
  *dn = v;
  if (zn) *zn = Zn;
  if (xn) *xn = Xn;
  if (yn) *yn = Yn;
  return ok;
}

// Where source pixel (x, y) with disparity d lands and with which value; false where it is dropped.
__host__ __device__ __forceinline__ bool reproject_pixel(const ReprojectArgs& a, float d, int x, int y, int* iu, int* iv,
                                                         float* dn) {
  double P[3];
  const bool ok = reproject_point(a.cam, a.min_disp, d, x, y, P);
  return reproject_project(a.cam, a.R, a.t, a.max_disp, a.rows, a.cols, ok, P, iu, iv, dn);
}

// The work of one thread of k_reproject_splat: source pixels x, x + 64, x + 128, x + 192 of row y.  The lanes of a wavefront
// hold consecutive x, so each of the four atomics of a wavefront falls on near-consecutive words (256 contiguous bytes where
// the motion keeps neighbours together): the shape at which memory-side atomics run at their full rate.  Four pixels of one
// 16-byte load per thread would put a wavefront's 64 words 16 bytes apart, four times as many 64-byte requests.
__host__ __device__ __forceinline__ void reproject_splat_lane(const ReprojectArgs& a, int x, int y) {
  const float* row = a.disp + (size_t)y * a.cols;
  float d[kReprojectPixelsPerLane];
#pragma unroll
  for (int k = 0; k < kReprojectPixelsPerLane; ++k) {
    const int xk = x + k * kReprojectLanes;
    d[k] = xk < a.cols ? row[xk] : 0.f;  // the four loads are in flight together
  }
#pragma unroll
  for (int k = 0; k < kReprojectPixelsPerLane; ++k) {
    int iu, iv;
    float dn;
    if (reproject_pixel(a, d[k], x + k * kReprojectLanes, y, &iu, &iv, &dn))  // 0 behind the row's end: takes no part
      reproject_raise(a.splat + ((size_t)iv * a.cols + iu), __builtin_bit_cast(unsigned, dn));
  }
}

// ---- stage 3: the closed left seed into the right view ----------------------------------------------------------------------
struct ReprojectRightArgs {
  const float* closed;  // C_l [rows][cols]: +0.0 or finite > 0
  int rows, cols;
  unsigned* splat;  // [rows][cols], zeroed
};

// The work of one thread of k_reproject_splat_right: pixels x, x + 64, x + 128, x + 192 of row y (as reproject_splat_lane).
__host__ __device__ __forceinline__ void reproject_right_lane(const ReprojectRightArgs& a, int x, int y) {
  const float* row = a.closed + (size_t)y * a.cols;
  float s[kReprojectPixelsPerLane];
#pragma unroll
  for (int k = 0; k < kReprojectPixelsPerLane; ++k) {
    const int xk = x + k * kReprojectLanes;
    s[k] = xk < a.cols ? row[xk] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < kReprojectPixelsPerLane; ++k) {
    const double q = __builtin_rint((double)(x + k * kReprojectLanes) - (double)s[k]);  // half to even
    if (s[k] > 0.f && q >= 0.0 && q < (double)a.cols)
      reproject_raise(a.splat + ((size_t)y * a.cols + (int)q), __builtin_bit_cast(unsigned, s[k]));
  }
}

// ---- stage 2: close and count, over a tile with an r-wide halo -----------------------------------------------------------------
struct ReprojectFinishArgs {
  const unsigned* in;  // S [rows][cols], the bits of a splat
  unsigned* out;       // C [rows][cols]; may be null (the call then only counts)
  int rows, cols, r;
  int* count;  // raised by the number of pixels > 0 of C
};

// Cell (lx, ly) of the staged region of the tile whose first pixel is (x0, y0), lx < kReprojectTileW + 2 r,
// ly < kReprojectTileH + 2 r: pixel (x0 - r + lx, y0 - r + ly), 0 outside the image.
__host__ __device__ __forceinline__ void reproject_stage_cell(const ReprojectFinishArgs& a, unsigned* tile, int lx, int ly,
                                                              int x0, int y0) {
  const int gx = x0 - a.r + lx, gy = y0 - a.r + ly;
  const bool inside = gx >= 0 && gx < a.cols && gy >= 0 && gy < a.rows;
  tile[ly * kReprojectTilePitch + lx] = inside ? a.in[(size_t)gy * a.cols + gx] : 0u;
}

// Pixel (lx, ly) of the tile, lx < kReprojectTileW, ly < kReprojectTileH: closes it, stores it, and says whether it is > 0.
// False and nothing stored outside the image.
__host__ __device__ __forceinline__ bool reproject_finish_pixel(const ReprojectFinishArgs& a, const unsigned* tile, int x0,
                                                                int y0, int lx, int ly) {
  const int gx = x0 + lx, gy = y0 + ly;
  if (gx >= a.cols || gy >= a.rows) return false;
  unsigned c = tile[(ly + a.r) * kReprojectTilePitch + lx + a.r];
  if (c == 0u) {
    const int n = 2 * a.r + 1;
    for (int dy = 0; dy < n; ++dy)
      for (int dx = 0; dx < n; ++dx) {
        const unsigned v = tile[(ly + dy) * kReprojectTilePitch + lx + dx];
        c = v > c ? v : c;
      }
  }
  if (a.out) a.out[(size_t)gy * a.cols + gx] = c;
  return c != 0u;
}

}  // namespace pm
