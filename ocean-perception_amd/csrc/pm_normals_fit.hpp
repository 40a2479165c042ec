// pm_normals_fit.hpp -- the kernel of pm_disparity_normals (include/pm/imaging.h); included by pm_stages.hip alone.  The
// staging, the per-pixel fit and the store are pm_normals_fit_body.hpp's, the definition is tests/normals_fit_ref.py
// (DESIGN.md section 8c-2).
//
// k_normals_fit<R>: a workgroup of kNormalsFitTileCols x kNormalsFitTileRows threads owns a tile of as many pixels, one
// per thread, one wavefront per tile row.  It stages the tile with a halo of r cells in LDS once (cells outside the image
// as 0.0f, which never counts), waits at ONE barrier that every thread reaches, and then each thread whose pixel lies in
// the image runs normals_fit_pixel over its (2r+1)^2 window: lanes read neighbouring floats of a tile row, so every LDS
// read is conflict-free.  A lane whose centre is not > 0 leaves the fit at once; a wavefront of such lanes skips the loop
// (the compiler branches on the empty exec mask).  No atomics, no wait between workgroups, no inline assembly.
// R = 1..7: the radius as a template constant, the window loops fully unrolled (pm_stages.hip dispatches).
#pragma once

#include <hip/hip_runtime.h>

#include "pm_normals_fit_body.hpp"

namespace pm {

constexpr int kNormalsFitThreads = kNormalsFitTileCols * kNormalsFitTileRows;

// grid = (ceil(cols / kNormalsFitTileCols), ceil(rows / kNormalsFitTileRows)), block = (kNormalsFitTileCols, kNormalsFitTileRows)
template <int R>
__global__ void __launch_bounds__(kNormalsFitThreads) k_normals_fit(NormalsFitArgs a) {
  static_assert(R >= 1 && R <= kNormalsFitMaxRadius, "radius 1..7");
  __shared__ float tile[normals_fit_tile_cells(R)];
  const int x0 = (int)blockIdx.x * kNormalsFitTileCols, y0 = (int)blockIdx.y * kNormalsFitTileRows;
  const int tid = (int)(threadIdx.y * kNormalsFitTileCols + threadIdx.x);
  normals_fit_stage(tile, R, a.disp, a.rows, a.cols, x0, y0, tid, kNormalsFitThreads);
  __syncthreads();
  const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
  if (x >= a.cols || y >= a.rows) return;  // behind the only barrier
  constexpr int pitch = normals_fit_tile_pitch(R);
  const float* centre = tile + ((int)threadIdx.y + R) * pitch + (int)threadIdx.x + R;
  normals_fit_store(a, x, y, normals_fit_pixel<R>(centre, pitch, R, a.max_diff, a.min_support));
}

#ifdef PM_TUNING
// The other side of the A/B recorded in DESIGN.md 8c-2 (tuning build only, PM_NORMALS_FIT_RUNTIME_RADIUS=1): ONE kernel
// with the radius as a launch argument, the tile sized for the largest radius, the window loops not unrolled.
__global__ void __launch_bounds__(kNormalsFitThreads) k_normals_fit_any(NormalsFitArgs a) {
  __shared__ float tile[normals_fit_tile_cells(kNormalsFitMaxRadius)];
  const int r = a.radius;
  const int x0 = (int)blockIdx.x * kNormalsFitTileCols, y0 = (int)blockIdx.y * kNormalsFitTileRows;
  const int tid = (int)(threadIdx.y * kNormalsFitTileCols + threadIdx.x);
  normals_fit_stage(tile, r, a.disp, a.rows, a.cols, x0, y0, tid, kNormalsFitThreads);
  __syncthreads();
  const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
  if (x >= a.cols || y >= a.rows) return;
  const int pitch = normals_fit_tile_pitch(r);
  const float* centre = tile + ((int)threadIdx.y + r) * pitch + (int)threadIdx.x + r;
  normals_fit_store(a, x, y, normals_fit_pixel<0>(centre, pitch, r, a.max_diff, a.min_support));
}
#endif

}  // namespace pm
