// pm_normals_fit_body.hpp -- the staging, the per-pixel plane fit and the store of pm_disparity_normals
// (include/pm/imaging.h), host-callable and free of kernels, so that the kernel (pm_normals_fit.hpp, in pm_stages.hip) and a
// CPU build (tests/cpp/normals_fit_host_main.cpp, under the sanitizers) share ONE statement of them.  The definition it is
// held to BIT FOR BIT is tests/normals_fit_ref.py: every operation is one rounding in the format
// written, parentheses and the order of the binary64 sums as written (the build uses -ffp-contract=off; binary64 add,
// multiply and divide are IEEE on gfx950).  The normal itself is pm_cloud_body.hpp's cloud_normal, not restated here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pm_cloud_body.hpp"

namespace pm {

constexpr int kNormalsFitTileCols = 64;   // pixels of a workgroup's tile along a row: one wavefront per tile row
constexpr int kNormalsFitTileRows = 8;    // ... and its rows
constexpr int kNormalsFitMaxRadius = 7;

// floats of a tile with its halo of r cells on every side
__host__ __device__ constexpr int normals_fit_tile_pitch(int r) { return kNormalsFitTileCols + 2 * r; }
__host__ __device__ constexpr int normals_fit_tile_cells(int r) {
  return normals_fit_tile_pitch(r) * (kNormalsFitTileRows + 2 * r);
}

// Thread `tid` of `threads` stages its share of the tile whose first pixel is (x0, y0): cell (tx, ty) of the tile holds
// disp(y0 - r + ty, x0 - r + tx), and 0.0f -- which never counts -- outside the image, so the tap loop has no bounds test.
__host__ __device__ __forceinline__ void normals_fit_stage(float* tile, int r, const float* disp, int rows, int cols, int x0,
                                                          int y0, int tid, int threads) {
  const int pitch = normals_fit_tile_pitch(r), cells = normals_fit_tile_cells(r);
  for (int i = tid; i < cells; i += threads) {
    const int ty = i / pitch, tx = i - ty * pitch;
    const int gx = x0 - r + tx, gy = y0 - r + ty;
    const bool inside = gx >= 0 && gx < cols && gy >= 0 && gy < rows;
    tile[i] = inside ? disp[(size_t)gy * cols + gx] : 0.f;
  }
}

struct NormalsFit {
  float a, b, z;  // the fitted plane at the pixel; meaningful where valid
  int support;    // the counting taps
  bool valid;
};

// The fit of the pixel at `c`, a cell of a zero-padded tile of pitch `pitch` with at least r cells on every side.
// R: the radius as a constant (the loops unroll), or 0 for the radius `r` of the call.
template <int R>
__host__ __device__ __forceinline__ NormalsFit normals_fit_pixel(const float* c, int pitch, int r, float max_diff,
                                                                 int min_support) {
  if (R) r = R;
  NormalsFit out = {0.f, 0.f, 0.f, 0, false};
  const float d0 = *c;
  if (!(d0 > 0.f)) return out;
  const double d064 = (double)d0, md = (double)max_diff;
  int n = 0, sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0;
  double se = 0.0, sxe = 0.0, sye = 0.0;
  // One window row at a time: with a constant R the taps of a row unroll (2R + 1 reads in flight), the rows do not --
  // unrolled too, the compiler hoists all (2R + 1)^2 reads and R = 7 spills.
#pragma unroll 1
  for (int dy = -r; dy <= r; ++dy) {
    const float* row = c + dy * pitch;
    int rn = 0, rsx = 0, rsxx = 0;
    double r0 = 0.0, r1 = 0.0;
#pragma unroll
    for (int dx = -r; dx <= r; ++dx) {
      const float t = row[dx];
      const double e = (double)t - d064;
      const bool k = t > 0.f && __builtin_fabs(e) <= md;  // false for a NaN e
      r0 = k ? r0 + e : r0;
      r1 = k ? r1 + ((double)dx * e) : r1;
      rn += k ? 1 : 0;
      rsx += k ? dx : 0;
      rsxx += k ? dx * dx : 0;
    }
    n += rn, sx += rsx, sxx += rsxx;
    sy += dy * rn, sxy += dy * rsx, syy += dy * dy * rn;
    se = se + r0;
    sxe = sxe + r1;
    sye = sye + ((double)dy * r0);
  }
  // cofactors of [[sxx, sxy, sx], [sxy, syy, sy], [sx, sy, n]]: 32 bits hold them for r <= 7, det needs 64
  const int c00 = syy * n - sy * sy, c01 = sx * sy - sxy * n, c02 = sxy * sy - syy * sx;
  const int c11 = sxx * n - sx * sx, c12 = sxy * sx - sxx * sy, c22 = sxx * syy - sxy * sxy;
  const long long det = (long long)sxx * c00 + (long long)sxy * c01 + (long long)sx * c02;
  out.support = n;
  out.valid = n >= min_support && det > 0;
  const double den = out.valid ? (double)det : 1.0;
  const double a64 = ((((double)c00 * sxe) + ((double)c01 * sye)) + ((double)c02 * se)) / den;
  const double b64 = ((((double)c01 * sxe) + ((double)c11 * sye)) + ((double)c12 * se)) / den;
  const double c64 = ((((double)c02 * sxe) + ((double)c12 * sye)) + ((double)c22 * se)) / den;
  out.a = (float)a64;
  out.b = (float)b64;
  out.z = (float)(d064 + c64);
  return out;
}

// One launch of pm_disparity_normals; a null output is not written.
struct NormalsFitArgs {
  CloudCam cam;  // read only where `normals` is given
  const float* disp;
  int rows, cols;
  int radius;
  float max_diff;
  int min_support;
  float* normals;    // [rows][cols][3]
  float* planes;     // [3][rows][cols]
  uint8_t* support;  // [rows][cols]
};

// The outputs of pixel (x, y), x < cols and y < rows: (0, 0, 0) planes and normal where the fit is not valid.
__host__ __device__ __forceinline__ void normals_fit_store(const NormalsFitArgs& a, int x, int y, const NormalsFit& f) {
  const size_t px = (size_t)y * a.cols + x, plane = (size_t)a.rows * a.cols;
  const float pa = f.valid ? f.a : 0.f, pb = f.valid ? f.b : 0.f, pz = f.valid ? f.z : 0.f;
  if (a.normals) {
    float n[3];
    cloud_normal(a.cam, pa, pb, pz, x, y, !f.valid, n);
    float* o = a.normals + px * 3;
    o[0] = n[0], o[1] = n[1], o[2] = n[2];
  }
  if (a.planes) {
    a.planes[px] = pa;
    a.planes[plane + px] = pb;
    a.planes[2 * plane + px] = pz;
  }
  if (a.support) a.support[px] = (uint8_t)f.support;
}

}  // namespace pm
