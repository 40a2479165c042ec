// pm_rectify.hpp -- undistortion + rectification of raw 8-bit frames in front of Match() (include/pm/imaging.h:
// pm_rectify_u8, pm_rectify_map, pm_match_raw_device; interleaved BGR through the same code: pm_rectify_bgr8,
// pm_match_raw_bgr_device).  The reference ships a calibration with non-zero distortion (config/shared/ACFR.yaml:27,48)
// and only warns that it does not undistort (src/vehicle/params/yaml_parser.cpp:153); this is the stage it lacks.  The definition the kernel is held to BIT FOR BIT is tests/rectify_ref.py (DESIGN.md
// section 8d): the project's own, not cv::remap's (OpenCV's 15-bit coefficient table is not reproduced).
//
// One kernel, no coordinate map in memory: a thread evaluates the radial-tangential model for four consecutive
// destination pixels of a row in registers -- binary64, one rounding per operation in the order written below (the build
// uses -ffp-contract=off; binary64 division is IEEE on gfx950; no fma, no rsqrt, no fast-math intrinsic) -- quantises the
// source position to 1/32 pixel, gathers the four source bytes of each pixel and blends them in integers.  The view
// (22 doubles) travels by value in the kernel arguments, so nothing is allocated or invalidated when a calibration
// changes, and a 720p pair moves 1.8 MB of image instead of reading 15 MB of map on top.  RectifyKind::Map makes the same
// code write the Q5 coordinates instead of the pixels: the map a test reads is the map the pixels were made from.
// Per pixel: about 60 binary64 operations and 3 divisions, 4 one-byte gathers, one byte out (two with the mask).
// Positions, inside test, weights, mask rule and the four-byte store are written once for every pixel format; a format has
// its own gather and its own pixel store, nothing else.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm/imaging.h"

namespace pm {

constexpr int kRectifyInvalid = INT32_MIN;  // both map entries of a pixel without a source position
constexpr int kRectifyBlockX = 64;          // threads along a row: 256 destination pixels
constexpr int kRectifyBlockY = 4;           // rows per block

// Q5 source position of the destination pixel whose normalised rectified coordinates are (a, b).  false: INVALID.
__host__ __device__ __forceinline__ bool rectify_source_q5(const pm_rectify_view& v, double a, double b, int* ix, int* iy) {
  // R^T (a, b, 1): back from the rectified into the raw camera's frame
  const double X = (v.R[0] * a + v.R[3] * b) + v.R[6];
  const double Y = (v.R[1] * a + v.R[4] * b) + v.R[7];
  const double W = (v.R[2] * a + v.R[5] * b) + v.R[8];
  const double x = X / W, y = Y / W;
  const double xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy;
  const pm_camera& c = v.cam;
  const double rad = 1.0 + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
  const double tx = ((2.0 * c.p1) * xy) + (c.p2 * (r2 + (2.0 * xx)));
  const double ty = (c.p1 * (r2 + (2.0 * yy))) + ((2.0 * c.p2) * xy);
  const double sx = c.fx * ((x * rad) + tx) + c.cx;
  const double sy = c.fy * ((y * rad) + ty) + c.cy;
  const double qx = sx * 32.0, qy = sy * 32.0;
  const double lim = 1073741824.0;  // 2^30; the comparisons are false for NaN
  const bool ok = (W > 0.0) && (fabs(qx) < lim) && (fabs(qy) < lim);
  // round half to even; a position that is not ok never reaches the conversion
  *ix = ok ? (int)rint(ok ? qx : 0.0) : kRectifyInvalid;
  *iy = ok ? (int)rint(ok ? qy : 0.0) : kRectifyInvalid;
  return ok;
}

// What a launch writes.  Gray: n gray images (+ mask).  Map: the Q5 coordinates, xy[(y * cols + x) * 2 + {0, 1}] =
// (ix, iy); src / dst / valid are not touched and the grid has z = 1.  Bgr: interleaved BGR, the 8-bit image (+ mask).
// BgrFloat: the float image = byte x (float)(1 / 255.) (CastImage3bTo3f), next to or instead of the 8-bit one (+ mask).
enum class RectifyKind { Gray, Map, Bgr, BgrFloat };

// The arguments of a launch, by value like the view inside them: filled once on the host, nothing allocated.
// src_step: bytes per source row (>= src_cols, BGR: >= 3 * src_cols).  Images follow one another at src_rows * src_step
// (source) and rows * cols pixels (destination, mask).  valid may be null; BgrFloat: dst may be null.
struct RectifyArgs {
  pm_rectify_view view;
  const uint8_t* src;
  int src_rows, src_cols;
  size_t src_step;
  int rows, cols;
  int border;
  uint8_t* dst;
  float* dstf;
  uint8_t* valid;
  int32_t* xy;
};

// ---- what does not depend on the pixel format --------------------------------------------------------------------------
// the Q5 source positions of destination pixels x4 .. x4 + 3 of row y
__host__ __device__ __forceinline__ void rectify_positions(const pm_rectify_view& view, int x4, int y, int ix[4], int iy[4],
                                                           bool ok[4]) {
  const double b = ((double)y - view.cy_new) / view.fy_new;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = ((double)(x4 + k) - view.cx_new) / view.fx_new;
    ok[k] = rectify_source_q5(view, a, b, &ix[k], &iy[k]);
  }
}
// in[t]: tap t (0 .. 3: x0, x0 + 1 of row y0, then of row y0 + 1) of pixel k of the thread is read from the image
__host__ __device__ __forceinline__ void rectify_inside(int ix, int iy, bool ok, int k, int count, int src_rows, int src_cols,
                                                        bool in[4]) {
  const int x0 = ix >> 5, y0 = iy >> 5;  // floor
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int tx = x0 + (t & 1), ty = y0 + (t >> 1);
    in[t] = ok && k < count && (unsigned)tx < (unsigned)src_cols && (unsigned)ty < (unsigned)src_rows;
  }
}
// the Q5 weights of the four taps (their sum is 1024)
__host__ __device__ __forceinline__ void rectify_weights(int ix, int iy, int w[4]) {
  const int ax = ix & 31, ay = iy & 31;
  w[0] = (32 - ax) * (32 - ay);
  w[1] = ax * (32 - ay);
  w[2] = (32 - ax) * ay;
  w[3] = ax * ay;
}
// the mask byte of a pixel: 255 where every tap with a non-zero weight came from the image
__host__ __device__ __forceinline__ unsigned rectify_mask_byte(bool ok, const bool in[4], const int w[4]) {
  bool all_in = ok;
#pragma unroll
  for (int t = 0; t < 4; ++t) all_in = all_in && (in[t] || w[t] == 0);
  return all_in ? 255u : 0u;
}
// The first `count` bytes of `word` (lowest first) to p: one 32-bit word where the address is 4-byte aligned and the row
// holds all four; byte stores otherwise (row tails, an unaligned destination, rows of a packed image whose width is no
// multiple of 4).
__host__ __device__ __forceinline__ void rectify_store4(uint8_t* p, unsigned word, int count) {
  if (count == 4 && ((uintptr_t)p & 3u) == 0) {
    *(uint32_t*)p = word;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < count) p[k] = (uint8_t)(word >> (8 * k));
  }
}

// ---- the gather of interleaved BGR (pm_rectify_bgr8, pm_match_raw_bgr_device) ---------------------------------------------
// The definition is tests/rectify_bgr_ref.py: the gray definition channel by channel at the SAME Q5 coordinates, one
// border value, one mask per image.  The geometry above is therefore evaluated once per destination pixel; the three
// channels share the position, the four weights and the mask.
//
// The two horizontally adjacent taps of a pixel are 6 contiguous bytes of a source row.  They are fetched as one 4-byte
// and one 2-byte access at byte alignment (the copies below become global_load_dword + global_load_ushort: global memory
// takes unaligned accesses on gfx950), 16 loads per thread like the gray kernel instead of 48 byte loads.  Nothing is read
// for a row of taps that lies outside the image altogether.  Where ONE of the two taps is inside -- x0 = -1 or
// x0 = src_cols - 1, the image's left and right edge -- the same 6-byte access is moved one pixel inwards (the window of
// columns xc, xc + 1 with xc = clamp(x0, 0, src_cols - 2)) and the tap is taken from the other half of it, so that every
// lane of a wave runs the same two loads, all eight pairs of a thread are in flight together, and no access reaches past
// byte 3 * src_cols of a row or past the allocation.  An image of ONE column has no such window: its only tap is read as
// 2 + 1 bytes (a branch every thread of the launch takes alike).

// The six bytes of one row of taps, loaded but not yet taken apart: a = bytes 0 .. 3, b = bytes 4 .. 5 of the window
// (src_cols == 1: a = bytes 0 .. 1, b = byte 2 of the only pixel).  in0 / in1: whether tap (x0, ty) / (x0 + 1, ty) is inside.
struct RectifyRaw {
  uint32_t a, b;
};
__host__ __device__ __forceinline__ RectifyRaw rectify_load_pair(const uint8_t* __restrict__ img, int src_cols, size_t src_step,
                                                                 int x0, int ty, bool in0, bool in1) {
  RectifyRaw r = {0u, 0u};
  if (in0 || in1) {
    const uint8_t* row = img + (size_t)ty * src_step;
    if (src_cols >= 2) {
      const int xc = x0 < 0 ? 0 : x0 > src_cols - 2 ? src_cols - 2 : x0;
      uint16_t hi;
      __builtin_memcpy(&r.a, row + (size_t)xc * 3, 4);
      __builtin_memcpy(&hi, row + (size_t)xc * 3 + 4, 2);
      r.b = hi;
    } else {
      uint16_t lo;
      __builtin_memcpy(&lo, row, 2);
      r.a = lo;
      r.b = row[2];
    }
  }
  return r;
}
// -> the left tap in bits 0 .. 23, the right one in bits 24 .. 47 (b | g << 8 | r << 16 each); a tap outside the image is
// `border3`, the border value in all three bytes
__host__ __device__ __forceinline__ uint64_t rectify_tap_pair(RectifyRaw r, int src_cols, int x0, bool in0, bool in1,
                                                              uint32_t border3) {
  uint32_t lo = r.a & 0xFFFFFFu, hi = (r.a >> 24) | (r.b << 8);  // columns xc and xc + 1 of the window
  if (src_cols < 2) lo = hi = r.a | (r.b << 16);
  const uint32_t left = !in0 ? border3 : x0 > src_cols - 2 ? hi : lo;  // x0 == src_cols - 1: the window moved left
  const uint32_t right = !in1 ? border3 : x0 < 0 ? lo : hi;            // x0 == -1: the window moved right
  return (uint64_t)left | ((uint64_t)right << 24);
}

// (w . taps + 512) >> 10 of channel c (0 .. 2) of the two tap pairs of a pixel
__host__ __device__ __forceinline__ unsigned rectify_blend(const int w[4], uint64_t top, uint64_t bot, int c) {
  const int sum = w[0] * (int)((top >> (8 * c)) & 255u) + w[1] * (int)((top >> (24 + 8 * c)) & 255u) +
                  w[2] * (int)((bot >> (8 * c)) & 255u) + w[3] * (int)((bot >> (24 + 8 * c)) & 255u);
  return (unsigned)((sum + 512) >> 10);
}

// ---- one thread, one kernel ---------------------------------------------------------------------------------------------
// The work of one thread: destination pixels x4 .. x4 + 3 of row y of image z (host-callable, so that a CPU build can
// run the kernel's own code).  Gray: four bytes of dst, stored by rectify_store4.  BGR: 12 bytes of dst as three 32-bit
// words under the rule of rectify_store4, byte by byte otherwise (the alignment of the rows of a packed image of odd width
// alternates); the 12 floats as three 16-byte stores under the same rule for 16 bytes.  The mask: four bytes, rectify_store4.
template <RectifyKind KIND>
__host__ __device__ __forceinline__ void rectify_four(const RectifyArgs& a, int x4, int y, int z) {
  constexpr bool BGR = KIND == RectifyKind::Bgr || KIND == RectifyKind::BgrFloat;
  const int count = a.cols - x4 < 4 ? a.cols - x4 : 4;
  int ix[4], iy[4];
  bool ok[4];
  rectify_positions(a.view, x4, y, ix, iy, ok);
  if constexpr (KIND == RectifyKind::Map) {
    int32_t* o = a.xy + ((size_t)y * a.cols + x4) * 2;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < count) {
        o[2 * k] = ix[k];
        o[2 * k + 1] = iy[k];
      }
    return;
  }
  const uint8_t* img = a.src + (size_t)z * a.src_rows * a.src_step;
  const int border = a.border;  // read once: a select below, no branch around each blend
  const uint32_t border3 = (uint32_t)border * 0x010101u;
  // the 16 gathers first (independent loads in flight together), the blends after them
  [[maybe_unused]] int tap[4][4];            // gray: the taps themselves
  [[maybe_unused]] RectifyRaw top[4], bot[4];  // BGR: the rows of taps, not yet taken apart
  bool in[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x0 = ix[k] >> 5, y0 = iy[k] >> 5;
    rectify_inside(ix[k], iy[k], ok[k], k, count, a.src_rows, a.src_cols, in[k]);
    if constexpr (BGR) {
      top[k] = rectify_load_pair(img, a.src_cols, a.src_step, x0, y0, in[k][0], in[k][1]);
      bot[k] = rectify_load_pair(img, a.src_cols, a.src_step, x0, y0 + 1, in[k][2], in[k][3]);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        tap[k][t] = in[k][t] ? (int)img[(size_t)(y0 + (t >> 1)) * a.src_step + (x0 + (t & 1))] : border;
    }
  }
  unsigned px[4], vm = 0;  // px[k]: the byte of pixel k; BGR: b | g << 8 | r << 16
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int w[4];
    rectify_weights(ix[k], iy[k], w);
    if constexpr (BGR) {
      const uint64_t t01 = rectify_tap_pair(top[k], a.src_cols, ix[k] >> 5, in[k][0], in[k][1], border3);
      const uint64_t t23 = rectify_tap_pair(bot[k], a.src_cols, ix[k] >> 5, in[k][2], in[k][3], border3);
      px[k] = ok[k] ? rectify_blend(w, t01, t23, 0) | (rectify_blend(w, t01, t23, 1) << 8) | (rectify_blend(w, t01, t23, 2) << 16)
                    : border3;
    } else {
      const int sum = w[0] * tap[k][0] + w[1] * tap[k][1] + w[2] * tap[k][2] + w[3] * tap[k][3];
      px[k] = ok[k] ? (unsigned)((sum + 512) >> 10) : (unsigned)border;
    }
    vm |= rectify_mask_byte(ok[k], in[k], w) << (8 * k);
  }
  const size_t at = ((size_t)z * a.rows + y) * a.cols + x4;
  if constexpr (!BGR) rectify_store4(a.dst + at, px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24), count);
  if (BGR && a.dst) {
    uint8_t* o = a.dst + at * 3;
    if (count == 4 && ((uintptr_t)o & 3u) == 0) {
      uint32_t* o32 = (uint32_t*)o;
      o32[0] = px[0] | (px[1] << 24);
      o32[1] = (px[1] >> 8) | (px[2] << 16);
      o32[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < count) {
          o[3 * k] = (uint8_t)px[k];
          o[3 * k + 1] = (uint8_t)(px[k] >> 8);
          o[3 * k + 2] = (uint8_t)(px[k] >> 16);
        }
    }
  }
  if constexpr (KIND == RectifyKind::BgrFloat) {
    const float s = (float)(1.0 / 255.0);
    float f[12];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) f[3 * k + c] = (float)((px[k] >> (8 * c)) & 255u) * s;
    float* o = a.dstf + at * 3;
    if (count == 4 && ((uintptr_t)o & 15u) == 0) {
      float4* o4 = (float4*)o;
      o4[0] = make_float4(f[0], f[1], f[2], f[3]);
      o4[1] = make_float4(f[4], f[5], f[6], f[7]);
      o4[2] = make_float4(f[8], f[9], f[10], f[11]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < count) {
          o[3 * k] = f[3 * k];
          o[3 * k + 1] = f[3 * k + 1];
          o[3 * k + 2] = f[3 * k + 2];
        }
    }
  }
  if (a.valid) rectify_store4(a.valid + at, vm, count);
}

// grid = (ceil(cols / 256), ceil(rows / 4), n), block = (64, 4).  A thread owns destination pixels x4 .. x4 + 3 of row y
// of image z.  Four instantiations, one per RectifyKind; Bgr compiles the float image out (dstf is not read): what
// pm_match_raw_bgr_device and every caller without a float image run.
template <RectifyKind KIND>
__global__ void __launch_bounds__(kRectifyBlockX * kRectifyBlockY) k_rectify(RectifyArgs a) {
  const int x4 = (int)(blockIdx.x * kRectifyBlockX + threadIdx.x) * 4;
  const int y = (int)(blockIdx.y * kRectifyBlockY + threadIdx.y);
  if (x4 >= a.cols || y >= a.rows) return;
  rectify_four<KIND>(a, x4, y, (int)blockIdx.z);
}

}  // namespace pm
