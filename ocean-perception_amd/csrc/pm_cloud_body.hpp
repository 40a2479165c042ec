// pm_cloud_body.hpp -- the per-pixel arithmetic and the per-thread bodies of the point-cloud stages (include/pm/imaging.h:
// pm_backproject, pm_planes_normals, pm_point_cloud), host-callable and free of kernels, so that the two translation units
// that use it (pm_stages.hip through pm_cloud.hpp, pm_planes_host.hip through pm_planes.hpp) and a CPU build
// (tests/cpp/cloud_host_main.cpp, under the sanitizers) share ONE statement of it.  The definition it is held to BIT FOR
// BIT is tests/pointcloud_ref.py: every operation is one rounding in the format written,
// parentheses as written (the build uses -ffp-contract=off; binary64 division is IEEE on gfx950; binary32 division and
// sqrt are correctly rounded through -fhip-fp32-correctly-rounded-divide-sqrt).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm/imaging.h"

namespace pm {

// the rectified pinhole of a launch: pm_cloud_camera with fx * baseline formed once on the host
struct CloudCam {
  double fx, fy, cx, cy, fxb;
};
inline CloudCam cloud_cam(const pm_cloud_camera& c) { return CloudCam{c.fx, c.fy, c.cx, c.cy, c.fx * c.baseline}; }

// The point of pixel (x, y) with disparity d; false and (0, 0, 0) where d is not > 0 (NaN included).  p[2] equals
// pm_disp_to_range's value (pm_imaging.hpp::disp_to_range) bit for bit.
__host__ __device__ __forceinline__ bool cloud_point(const CloudCam& c, float d, int x, int y, float p[3]) {
  const bool ok = d > 0.f;
  const double Zd = c.fxb / (double)(ok ? d : 1.f);
  const double Xd = (((double)x - c.cx) * Zd) / c.fx;
  const double Yd = (((double)y - c.cy) * Zd) / c.fy;
  p[0] = ok ? (float)Xd : 0.f;
  p[1] = ok ? (float)Yd : 0.f;
  p[2] = ok ? (float)Zd : 0.f;
  return ok;
}

// pm_cloud_filter's rule for a pixel on the stride grid: d > 0 (`ok` of cloud_point), d >= min_disp, and the point's Z
// within max_range where that is not 0.  Every comparison is false for NaN.
__host__ __device__ __forceinline__ bool cloud_counts(const pm_cloud_filter& f, bool ok, float d, float z) {
  return ok && d >= f.min_disp && (f.max_range == 0.f || z <= f.max_range);
}

// The unit normal, facing the camera, of the plane (a, b, z) stored for pixel (x, y): disparity a (u - x) + b (v - y) + z
// at pixel (u, v).  (0, 0, 0) where z is not > 0, where `masked`, and where the length is not finite or not > 0.
__host__ __device__ __forceinline__ void cloud_normal(const CloudCam& c, float a, float b, float z, int x, int y, bool masked,
                                                      float n[3]) {
  const double a64 = (double)a, b64 = (double)b;
  const float nx = (float)(a64 * c.fx);
  const float ny = (float)(b64 * c.fy);
  const float nz = (float)((double)z - ((a64 * ((double)x - c.cx)) + (b64 * ((double)y - c.cy))));
  const float s = ((nx * nx) + (ny * ny)) + (nz * nz);
  const float l = __builtin_sqrtf(s);
  const bool ok = z > 0.f && !masked && l > 0.f && l < __builtin_inff();
  const float q = ok ? l : 1.f;
  n[0] = ok ? -(nx / q) : 0.f;
  n[1] = ok ? -(ny / q) : 0.f;
  n[2] = ok ? -(nz / q) : 0.f;
}

// ---- the per-thread bodies of pm_cloud.hpp's kernels ---------------------------------------------------------------------
struct BackprojectArgs {
  CloudCam cam;
  const float* disp;
  int rows, cols;
  float* xyz;
};

// The work of one thread of k_backproject: pixels x4 .. x4 + 3 of row y (host-callable: a CPU build runs it under the
// sanitizers, tests/cpp/cloud_host_main.cpp).
__host__ __device__ __forceinline__ void backproject_four(const BackprojectArgs& a, int x4, int y) {
  const int count = a.cols - x4 < 4 ? a.cols - x4 : 4;
  const float* in = a.disp + (size_t)y * a.cols + x4;
  float d[4] = {0.f, 0.f, 0.f, 0.f};
  if (count == 4 && ((uintptr_t)in & 15u) == 0) {
    const float4 v = *(const float4*)in;
    d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < count) d[k] = in[k];
  }
  float f[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) cloud_point(a.cam, d[k], x4 + k, y, f + 3 * k);
  float* o = a.xyz + ((size_t)y * a.cols + x4) * 3;
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

// What the count and the scatter launch share.  sub_cols: columns of the stride grid, items: its size.
struct CloudArgs {
  CloudCam cam;
  pm_cloud_filter filter;
  const float* disp;
  int rows, cols, sub_cols;
  long long items;
};

// The stride grid of a rows x cols map (host only): cloud_grid of the rows and of the columns, and the launch's arguments.
inline int cloud_grid(int n, int stride) { return (n + stride - 1) / stride; }
inline CloudArgs cloud_args(const pm_cloud_camera& camera, const pm_cloud_filter& filter, const float* d_disp, int rows,
                            int cols) {
  const int sub_rows = cloud_grid(rows, filter.stride), sub_cols = cloud_grid(cols, filter.stride);
  return CloudArgs{cloud_cam(camera), filter, d_disp, rows, cols, sub_cols, (long long)sub_rows * sub_cols};
}

// Item `item` of the stride grid: its pixel, its point, and whether it counts.  item < a.items.
__host__ __device__ __forceinline__ bool cloud_item(const CloudArgs& a, long long item, int* x, int* y, float p[3]) {
  const int ys = (int)(item / a.sub_cols), xs = (int)(item - (long long)ys * a.sub_cols);
  *x = xs * a.filter.stride;
  *y = ys * a.filter.stride;
  const float d = a.disp[(size_t)*y * a.cols + *x];
  const bool ok = cloud_point(a.cam, d, *x, *y, p);
  return cloud_counts(a.filter, ok, d, p[2]);
}

// the optional streams of the scatter: organised inputs, compacted outputs (a null output is not written)
struct CloudStreams {
  const float* normals;
  const uint8_t* bgr8;
  float* xyz_out;
  float* normals_out;
  uint8_t* bgr8_out;
  int32_t* index_out;
  int capacity;
};

// One counted item into its slot (host-callable, like backproject_four).
__host__ __device__ __forceinline__ void cloud_store(const CloudArgs& a, const CloudStreams& s, long long slot, int x, int y,
                                                     const float p[3]) {
  const size_t px = (size_t)y * a.cols + x;
  if (s.xyz_out) {
    float* o = s.xyz_out + (size_t)slot * 3;
    o[0] = p[0], o[1] = p[1], o[2] = p[2];
  }
  if (s.normals_out) {
    const float* n = s.normals + px * 3;
    float* o = s.normals_out + (size_t)slot * 3;
    o[0] = n[0], o[1] = n[1], o[2] = n[2];
  }
  if (s.bgr8_out) {
    const uint8_t* c = s.bgr8 + px * 3;
    uint8_t* o = s.bgr8_out + (size_t)slot * 3;
    o[0] = c[0], o[1] = c[1], o[2] = c[2];
  }
  if (s.index_out) s.index_out[slot] = (int32_t)px;
}

}  // namespace pm
