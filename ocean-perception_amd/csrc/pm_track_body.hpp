// pm_track_body.hpp -- the scalar pieces of pm_track_features (include/pm/imaging.h), host-callable and free of kernels, so
// that the kernels (pm_track.hpp) and a CPU build (tests/cpp/motion_main.cpp, under the sanitizers) share ONE statement of
// them.  The definition they are held to BIT FOR BIT is tests/motion_ref.py.  Everything up to the
// prediction is exact integer arithmetic; the prediction is pm_reproject_disparity's (pm_reproject_body.hpp:
// reproject_point, then `splat`'s projection without its image test); the sub-pixel step is one binary64 division, one
// addition and one rounding to binary32.
//
// Layouts the pieces agree on (a workgroup's LDS on the device, plain arrays on the host):
//   image tile     (cell + 8)^2 bytes, pitch cell + 8: the cell with a 4-pixel halo, 0 outside the image
//   gradient tile  (cell + 6)^2 TrackGrad, pitch cell + 6: entry (lx, ly) is the Sobel pair of image-tile pixel (lx + 1, ly + 1)
//   template       (2p + 1) rows of kTrackTmplPitchW words: the row's bytes, little endian, 0 behind its end
//   search region  (2s + 2p + 1) rows of track_region_pitch() words: bytes of the new image, 0 outside it and behind the row's
//                  end; two spare words per row, so that the aligned pair of words around any 4 bytes of a patch row is there
//   SAD table      (2s + 1)^2 uint16, row-major: kTrackNoSad where the candidate does not count (the largest SAD is 57 375)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_reproject_body.hpp"

namespace pm {

constexpr int kTrackHalo = 4;         // Sobel (1) inside the 7x7 window (3)
constexpr int kTrackMinCell = 8, kTrackMaxCell = 64;
constexpr int kTrackMaxPatch = 7;     // p
constexpr int kTrackMaxSearch = 24;   // s
constexpr int kTrackTmplPitchW = 4;   // 16 bytes hold the 15 of the widest template row
constexpr int kTrackMaxRegion = 2 * kTrackMaxSearch + 2 * kTrackMaxPatch + 1;  // 63
constexpr int kTrackMaxRegionPitchW = (kTrackMaxRegion + 3) / 4 + 2;           // 18
constexpr int kTrackMaxCandidates = (2 * kTrackMaxSearch + 1) * (2 * kTrackMaxSearch + 1);  // 2401 < 4096
constexpr unsigned kTrackNoSad = 0xFFFFu;
constexpr unsigned kTrackNoKey = 0xFFFFFFFFu;
constexpr int kTrackNone = INT32_MAX;  // sad / second of a record without one

struct TrackGrad {
  short gx, gy;  // |g| <= 1020
};

struct TrackOpt {  // pm_track_options, checked
  int cell, p, s;
  long long min_score;
  float min_disp, max_disp;
  int max_sad, min_gap;
};

// ---- select ------------------------------------------------------------------------------------------------------------------
// The Sobel pair of pixel (lx, ly) of an image tile, 1 <= lx, ly and lx + 1, ly + 1 inside the tile.
__host__ __device__ __forceinline__ TrackGrad track_sobel(const uint8_t* tile, int pitch, int lx, int ly) {
  const uint8_t* a = tile + (ly - 1) * pitch + lx;
  const uint8_t* b = a + pitch;
  const uint8_t* c = b + pitch;
  const int gx = ((int)a[1] + 2 * (int)b[1] + (int)c[1]) - ((int)a[-1] + 2 * (int)b[-1] + (int)c[-1]);
  const int gy = ((int)c[-1] + 2 * (int)c[0] + (int)c[1]) - ((int)a[-1] + 2 * (int)a[0] + (int)a[1]);
  return TrackGrad{(short)gx, (short)gy};
}

// The score of the pixel whose gradient-tile entry is (lx, ly), 3 <= lx, ly and lx + 3, ly + 3 inside the tile: Harris with
// k = 1 / 16 over the 7x7 window, exact.  The three sums are at most 49 * 1020^2 < 2^26.
__host__ __device__ __forceinline__ long long track_score(const TrackGrad* grad, int pitch, int lx, int ly) {
  int sxx = 0, syy = 0, sxy = 0;
  for (int dy = -3; dy <= 3; ++dy) {
    const TrackGrad* row = grad + (ly + dy) * pitch + lx;
#pragma unroll
    for (int dx = -3; dx <= 3; ++dx) {
      const int gx = row[dx].gx, gy = row[dx].gy;
      sxx += gx * gx;
      syy += gy * gy;
      sxy += gx * gy;
    }
  }
  const long long xx = sxx, yy = syy, xy = sxy;
  return 16 * (xx * yy - xy * xy) - (xx + yy) * (xx + yy);
}

// Everything of `eligible` but the score: the margin m = max(p, 4) and the disparity.
__host__ __device__ __forceinline__ bool track_eligible(const TrackOpt& o, int rows, int cols, int x, int y, float d) {
  const int m = o.p > kTrackHalo ? o.p : kTrackHalo;
  const bool inside = x >= m && x <= cols - 1 - m && y >= m && y <= rows - 1 - m;
  const bool finite = d < __builtin_inff();  // d > 0 below: false for NaN, and -inf is not > 0
  return inside && d > 0.f && finite && d >= o.min_disp && (o.max_disp == 0.f || d <= o.max_disp);
}

// Whether (score, index) beats (best_score, best_index): the larger score, a tie to the smaller index; index < 0 is "none".
__host__ __device__ __forceinline__ bool track_better(long long score, int index, long long best_score, int best_index) {
  return index >= 0 && (best_index < 0 || score > best_score || (score == best_score && index < best_index));
}

// ---- predict -----------------------------------------------------------------------------------------------------------------
// Pixel (x, y) of the old image with disparity d > 0 through X_new = R X + t: the pixel of the new image it is expected at,
// which may lie outside that image.  False, and (0, 0), unless Zn > 0 and |u|, |v| < 2^30.
__host__ __device__ __forceinline__ bool track_predict(const CloudCam& c, const double R[9], const double t[3], float d, int x,
                                                       int y, int* iu, int* iv) {
  double P[3];
  reproject_point(c, 0.f, d, x, y, P);
  const double X = P[0], Y = P[1], Z = P[2];
  const double Xn = (((R[0] * X) + (R[1] * Y)) + (R[2] * Z)) + t[0];
  const double Yn = (((R[3] * X) + (R[4] * Y)) + (R[5] * Z)) + t[1];
  const double Zn = (((R[6] * X) + (R[7] * Y)) + (R[8] * Z)) + t[2];
  const double u = (c.fx * (Xn / Zn)) + c.cx;
  const double v = (c.fy * (Yn / Zn)) + c.cy;
  const double lim = 1073741824.0;  // 2^30
  const bool ok = Zn > 0.0 && __builtin_fabs(u) < lim && __builtin_fabs(v) < lim;
  *iu = ok ? (int)__builtin_rint(u) : 0;  // half to even
  *iv = ok ? (int)__builtin_rint(v) : 0;
  return ok;
}

// ---- match -------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int track_region_pitch(int p, int s) { return (2 * s + 2 * p + 1 + 3) / 4 + 2; }

// Word j of row dy of the template of feature (x, y): bytes 4j .. 4j + 3 of the row, 0 behind byte 2p.  The feature is
// eligible, so the whole patch lies inside the image.
__host__ __device__ __forceinline__ unsigned track_tmpl_word(const uint8_t* old, int cols, int x, int y, int p, int j, int dy) {
  const uint8_t* row = old + (size_t)(y - p + dy) * cols + (x - p);
  unsigned w = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int i = 4 * j + b;
    if (i <= 2 * p) w |= (unsigned)row[i] << (8 * b);
  }
  return w;
}

// Word j of row ly of the search region whose first byte is pixel (x0, y0) of the new image and whose rows hold `width` bytes.
__host__ __device__ __forceinline__ unsigned track_region_word(const uint8_t* img, int rows, int cols, int x0, int y0, int width,
                                                               int j, int ly) {
  const int gy = y0 + ly;
  if (gy < 0 || gy >= rows) return 0u;
  const uint8_t* row = img + (size_t)gy * cols;
  unsigned w = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int lx = 4 * j + b, gx = x0 + lx;
    if (lx < width && gx >= 0 && gx < cols) w |= (unsigned)row[gx] << (8 * b);
  }
  return w;
}

// acc + the sum of the absolute differences of the four bytes of a and b: v_sad_u8 on the device
__host__ __device__ __forceinline__ unsigned track_sad4(unsigned a, unsigned b, unsigned acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sad_u8(a, b, acc);
#else
  for (int k = 0; k < 4; ++k) {
    const int d = (int)((a >> (8 * k)) & 255u) - (int)((b >> (8 * k)) & 255u);
    acc += (unsigned)(d < 0 ? -d : d);
  }
  return acc;
#endif
}

// the four bytes that start `shift` (0 .. 3) bytes into the pair of words (lo, hi): v_alignbyte_b32 on the device
__host__ __device__ __forceinline__ unsigned track_align(unsigned hi, unsigned lo, unsigned shift) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, shift);
#else
  return (unsigned)((((unsigned long long)hi << 32) | lo) >> (8 * shift));
#endif
}

// The SAD of the candidate whose patch starts at byte (cx, cy) of the region: four bytes at a time, the last word of a row
// masked to the bytes the row has (the template is 0 there).
__host__ __device__ __forceinline__ unsigned track_sad(const unsigned* tmpl, const unsigned* region, int pitch_w, int p, int cx,
                                                       int cy) {
  const int n = 2 * p + 1, nw = (n + 3) >> 2;
  const unsigned last = (1u << (8 * (n & 3))) - 1u;  // n is odd: 1 or 3 bytes
  unsigned acc = 0;
  for (int dy = 0; dy < n; ++dy) {
    const unsigned* trow = tmpl + dy * kTrackTmplPitchW;
    const unsigned* rrow = region + (cy + dy) * pitch_w;
    for (int j = 0; j < nw; ++j) {
      const int at = cx + 4 * j, w = at >> 2;
      unsigned v = track_align(rrow[w + 1], rrow[w], (unsigned)(at & 3));
      if (j == nw - 1) v &= last;
      acc = track_sad4(trow[j], v, acc);
    }
  }
  return acc;
}

// Whether candidate (ex, ey) of the window around (iu, iv) counts: its patch lies inside the new image.
__host__ __device__ __forceinline__ bool track_counts(int rows, int cols, int p, int qx, int qy) {
  return qx - p >= 0 && qx + p < cols && qy - p >= 0 && qy + p < rows;
}

// The key the workgroup minimises: the first of the smallest SADs wins without a second pass.
__host__ __device__ __forceinline__ unsigned track_key(unsigned sad, int index) { return (sad << 12) | (unsigned)index; }

// Whether candidate c lies at Chebyshev distance >= 2 from candidate `best` in a window of n1 columns.
__host__ __device__ __forceinline__ bool track_far(int c, int best, int n1) {
  const int cy = c / n1, by = best / n1;
  const int dy = cy - by, dx = (c - cy * n1) - (best - by * n1);
  return dy >= 2 || dy <= -2 || dx >= 2 || dx <= -2;
}

// ---- sub-pixel and the record ------------------------------------------------------------------------------------------------
// The position along one axis: q, moved by the vertex of the parabola through (cm, c0, cp) where both neighbours count
// (neither is kTrackNoSad), it opens upwards and the match is not perfect (c0 > 0: a perfect match stays on its pixel).
__host__ __device__ __forceinline__ float track_subpix(int q, unsigned cm, unsigned c0, unsigned cp, bool* used) {
  const int den = (int)cm - 2 * (int)c0 + (int)cp;
  *used = cm != kTrackNoSad && cp != kTrackNoSad && den > 0 && c0 > 0u;
  const double off = (double)((int)cm - (int)cp) / (double)(2 * (*used ? den : 1));
  return *used ? (float)((double)q + off) : (float)q;
}

// The record of a feature that was not predicted.
__host__ __device__ __forceinline__ void track_unpredicted(int x, int y, float d, pm_track* r) {
  r->x = x, r->y = y, r->disp = d;
  r->x_new = 0.f, r->y_new = 0.f;
  r->sad = kTrackNone, r->second = kTrackNone;
  r->flags = 0u;
}

// The record of a predicted feature from its finished SAD table: `key` the smallest key (kTrackNoKey: no candidate counts),
// `second` the smallest SAD at Chebyshev distance >= 2 from the best (kTrackNoSad: none).
__host__ __device__ __forceinline__ void track_finish(const TrackOpt& o, const uint16_t* table, int iu, int iv, unsigned key,
                                                      unsigned second, int x, int y, float d, pm_track* r) {
  r->x = x, r->y = y, r->disp = d;
  if (key == kTrackNoKey) {
    r->x_new = (float)iu, r->y_new = (float)iv;
    r->sad = kTrackNone, r->second = kTrackNone;
    r->flags = PM_TRACK_PREDICTED;
    return;
  }
  const int n1 = 2 * o.s + 1;
  const int best = (int)(key & 4095u), by = best / n1, bx = best - by * n1;
  const unsigned c0 = key >> 12;
  const unsigned xm = bx > 0 ? table[best - 1] : kTrackNoSad, xp = bx < n1 - 1 ? table[best + 1] : kTrackNoSad;
  const unsigned ym = by > 0 ? table[best - n1] : kTrackNoSad, yp = by < n1 - 1 ? table[best + n1] : kTrackNoSad;
  bool ux, uy;
  r->x_new = track_subpix(iu - o.s + bx, xm, c0, xp, &ux);
  r->y_new = track_subpix(iv - o.s + by, ym, c0, yp, &uy);
  const int sad = (int)c0, sec = second == kTrackNoSad ? kTrackNone : (int)second;
  r->sad = sad, r->second = sec;
  unsigned f = PM_TRACK_PREDICTED | PM_TRACK_MATCHED | (ux ? PM_TRACK_SUBPIX_X : 0u) | (uy ? PM_TRACK_SUBPIX_Y : 0u);
  if (o.max_sad != 0 && sad > o.max_sad) f |= PM_TRACK_FAIL_SAD;
  if (sec != kTrackNone && sec - sad < o.min_gap) f |= PM_TRACK_FAIL_GAP;
  r->flags = f;
}

}  // namespace pm
