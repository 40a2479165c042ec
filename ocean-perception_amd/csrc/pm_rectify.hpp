// pm_rectify.hpp -- undistortion + rectification of raw 8-bit frames in front of Match() (include/pm/imaging.h:
// pm_rectify_u8, pm_rectify_map, pm_match_raw_device).  The reference ships a calibration with non-zero distortion
// (config/shared/ACFR.yaml:27,48) and only warns that it does not undistort (src/vehicle/params/yaml_parser.cpp:153);
// this is the stage it lacks.  The definition the kernel is held to BIT FOR BIT is tests/rectify_ref.py (DESIGN.md
// section 8d): the project's own, not cv::remap's (OpenCV's 15-bit coefficient table is not reproduced).
//
// One kernel, no coordinate map in memory: a thread evaluates the radial-tangential model for four consecutive
// destination pixels of a row in registers -- binary64, one rounding per operation in the order written below (the build
// uses -ffp-contract=off; binary64 division is IEEE on gfx950; no fma, no rsqrt, no fast-math intrinsic) -- quantises the
// source position to 1/32 pixel, gathers the four source bytes of each pixel and blends them in integers.  The view
// (22 doubles) travels by value in the kernel arguments, so nothing is allocated or invalidated when a calibration
// changes, and a 720p pair moves 1.8 MB of image instead of reading 15 MB of map on top.  MAP = true makes the same
// code write the Q5 coordinates instead of the pixels: the map a test reads is the map the pixels were made from.
// Per pixel: about 60 binary64 operations and 3 divisions, 4 one-byte gathers, one byte out (two with the mask).
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

// grid = (ceil(cols / 256), ceil(rows / 4), n), block = (64, 4).  A thread owns destination pixels x4 .. x4 + 3 of row y
// of image z and stores them as one 32-bit word where the address is 4-byte aligned and the row holds all four; byte
// stores otherwise (row tails, unaligned d_dst, rows of a packed image whose width is no multiple of 4).
// MAP: xy[(y * cols + x) * 2 + {0, 1}] = (ix, iy) instead; src / dst / valid are not touched and the grid has z = 1.
// The work of one thread: destination pixels x4 .. x4 + 3 of row y of image z (host-callable, so that a CPU build can
// run the kernel's own code).
template <bool MAP>
__host__ __device__ __forceinline__ void rectify_four(const pm_rectify_view& view, const uint8_t* __restrict__ src,
                                                      int src_rows, int src_cols, size_t src_step, int rows, int cols,
                                                      int border, uint8_t* __restrict__ dst, uint8_t* __restrict__ valid,
                                                      int32_t* __restrict__ xy, int x4, int y, int z) {
  const int count = cols - x4 < 4 ? cols - x4 : 4;
  const double b = ((double)y - view.cy_new) / view.fy_new;
  int ix[4], iy[4];
  bool ok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = ((double)(x4 + k) - view.cx_new) / view.fx_new;
    ok[k] = rectify_source_q5(view, a, b, &ix[k], &iy[k]);
  }
  if (MAP) {
    int32_t* o = xy + ((size_t)y * cols + x4) * 2;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < count) {
        o[2 * k] = ix[k];
        o[2 * k + 1] = iy[k];
      }
    return;
  }
  const uint8_t* img = src + (size_t)z * src_rows * src_step;
  // the 16 gathers first (independent loads in flight together), the blends after them
  int tap[4][4];
  bool in[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x0 = ix[k] >> 5, y0 = iy[k] >> 5;  // floor
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int tx = x0 + (t & 1), ty = y0 + (t >> 1);
      in[k][t] = ok[k] && k < count && (unsigned)tx < (unsigned)src_cols && (unsigned)ty < (unsigned)src_rows;
      tap[k][t] = in[k][t] ? (int)img[(size_t)ty * src_step + tx] : border;
    }
  }
  unsigned px = 0, vm = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ax = ix[k] & 31, ay = iy[k] & 31;
    const int w[4] = {(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay};
    const int sum = w[0] * tap[k][0] + w[1] * tap[k][1] + w[2] * tap[k][2] + w[3] * tap[k][3];
    bool all_in = ok[k];
#pragma unroll
    for (int t = 0; t < 4; ++t) all_in = all_in && (in[k][t] || w[t] == 0);
    const unsigned out = ok[k] ? (unsigned)((sum + 512) >> 10) : (unsigned)border;
    px |= out << (8 * k);
    vm |= (all_in ? 255u : 0u) << (8 * k);
  }
  const size_t at = ((size_t)z * rows + y) * cols + x4;
  uint8_t* o = dst + at;
  if (count == 4 && ((uintptr_t)o & 3u) == 0) {
    *(uint32_t*)o = px;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < count) o[k] = (uint8_t)(px >> (8 * k));
  }
  if (valid) {
    uint8_t* m = valid + at;
    if (count == 4 && ((uintptr_t)m & 3u) == 0) {
      *(uint32_t*)m = vm;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < count) m[k] = (uint8_t)(vm >> (8 * k));
    }
  }
}

template <bool MAP>
__global__ void __launch_bounds__(kRectifyBlockX * kRectifyBlockY)
    k_rectify(pm_rectify_view view, const uint8_t* __restrict__ src, int src_rows, int src_cols, size_t src_step, int rows,
              int cols, int border, uint8_t* __restrict__ dst, uint8_t* __restrict__ valid, int32_t* __restrict__ xy) {
  const int x4 = (int)(blockIdx.x * kRectifyBlockX + threadIdx.x) * 4;
  const int y = (int)(blockIdx.y * kRectifyBlockY + threadIdx.y);
  if (x4 >= cols || y >= rows) return;
  rectify_four<MAP>(view, src, src_rows, src_cols, src_step, rows, cols, border, dst, valid, xy, x4, y, (int)blockIdx.z);
}

}  // namespace pm
