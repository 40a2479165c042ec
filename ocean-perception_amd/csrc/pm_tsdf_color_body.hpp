// pm_tsdf_color_body.hpp -- the per-voxel, per-pixel and per-point arithmetic and the per-thread bodies of
// pm_tsdf_integrate_color, pm_tsdf_color_map and pm_tsdf_color_points (include/pm/imaging.h), host-callable and free of kernels,
// so that the kernels (pm_tsdf_color.hpp) and a CPU build (tests/cpp/tsdf_color_host_main.cpp, under the sanitizers) share ONE
// statement of it.  The definition it is held to BIT FOR BIT is tests/tsdf_color_ref.py: every
// operation is one rounding in the format written, parentheses as written.  The distance half of the integrate is
// pm_tsdf_body.hpp's tsdf_integrate_lane itself, given the colour update as its `more`; the rays of the map gather are that
// header's tsdf_ray_direction and tsdf_ray_point.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_tsdf_body.hpp"

namespace pm {

// One colour record: 16 bytes, one load and one store.  weight == 0: never coloured.
struct alignas(16) TsdfColor {
  float b, g, r, weight;
};

typedef float TsdfColorWords __attribute__((ext_vector_type(4)));  // a record as the gathers load it

// finite: neither NaN nor +-inf (x - x is +0.0 for every finite x and NaN otherwise)
__host__ __device__ __forceinline__ bool tsdf_color_finite(float x) { return (x - x) == 0.f; }

// ---- integrate ----------------------------------------------------------------------------------------------------------------
// The launch's one argument, by value: pm_tsdf_integrate's own (its counts now int[3]: in view, updated, coloured) and the
// colour's.  Exactly one of bgr8 and bgr is given.
struct TsdfIntegrateColorArgs {
  TsdfIntegrateArgs base;
  double bandw;         // (double)band * trunc, formed on the host
  const uint8_t* bgr8;  // [rows][cols][3]
  const float* bgr;     // [rows][cols][3]
  TsdfColor* colors;    // [nz][ny][nx]
};

// What an updated voxel does beyond its distance record: inside the band, and with a finite pixel, the running weighted mean of
// its colour record.  The record and the pixel are touched only then.  Returns bit 2: coloured.
struct TsdfColorUpdate {
  const TsdfIntegrateColorArgs& a;
  __host__ __device__ __forceinline__ unsigned operator()(size_t voxel, size_t px, double sdf, float wn) const {
    if (!(sdf <= a.bandw && sdf >= -a.bandw)) return 0u;
    float p[3];
    if (a.bgr8) {
      const uint8_t* const at = a.bgr8 + 3 * px;
      p[0] = (float)at[0], p[1] = (float)at[1], p[2] = (float)at[2];
    } else {
      const float* const at = a.bgr + 3 * px;
      p[0] = at[0], p[1] = at[1], p[2] = at[2];
      if (!(tsdf_color_finite(p[0]) && tsdf_color_finite(p[1]) && tsdf_color_finite(p[2]))) return 0u;
    }
    TsdfColor* const at = a.colors + voxel;
    const TsdfColor v = *at;  // one 16-byte load ...
    TsdfColor o;
    o.b = ((v.b * v.weight) + (p[0] * wn)) / (v.weight + wn);
    o.g = ((v.g * v.weight) + (p[1] * wn)) / (v.weight + wn);
    o.r = ((v.r * v.weight) + (p[2] * wn)) / (v.weight + wn);
    o.weight = __builtin_fminf(v.weight + wn, a.base.grid.max_weight);
    *at = o;  // ... and one 16-byte store
    return 4u;
  }
};

// The work of one thread of k_tsdf_integrate_color: voxel (i, j, k), inside the grid.  Bit 0: in view, bit 1: updated, bit 2:
// coloured.
__host__ __device__ __forceinline__ unsigned tsdf_integrate_color_lane(const TsdfIntegrateColorArgs& a, int i, int j, int k) {
  return tsdf_integrate_lane(a.base, i, j, k, TsdfColorUpdate{a});
}

// ---- the two gathers ----------------------------------------------------------------------------------------------------------
// What both gathers are given.
struct TsdfColorSampler {
  TsdfGrid grid;
  float min_weight, byte_scale;
  const TsdfColor* colors;
  float* bgr_out;     // [n][3]; may be null
  uint8_t* bgr8_out;  // [n][3]; may be null
  int* counts;        // [0] coloured; zeroed
};

// The normalised trilinear mean of the colour volume at grid coordinates q; false where no corner takes part.  A corner outside
// the grid is never read; there is no test on the point itself.
__host__ __device__ __forceinline__ bool tsdf_color_sample(const TsdfColorSampler& s, const double q[3], float value[3]) {
  const double limit = 1073741824.0;  // 2^30: NaN and +-inf fail the comparison
  if (!(__builtin_fabs(q[0]) < limit && __builtin_fabs(q[1]) < limit && __builtin_fabs(q[2]) < limit)) return false;
  const TsdfGrid& g = s.grid;
  const double l0 = __builtin_floor(q[0]), l1 = __builtin_floor(q[1]), l2 = __builtin_floor(q[2]);
  const float f0 = (float)(q[0] - l0), f1 = (float)(q[1] - l1), f2 = (float)(q[2] - l2);
  const int i0 = (int)l0, i1 = (int)l1, i2 = (int)l2;
  const float w0[2] = {1.0f - f0, f0}, w1[2] = {1.0f - f1, f1}, w2[2] = {1.0f - f2, f2};
  float den = 0.f, num[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int bx = c & 1, by = (c >> 1) & 1, bz = c >> 2;
    const int x = i0 + bx, y = i1 + by, z = i2 + bz;
    if (x < 0 || x >= g.nx || y < 0 || y >= g.ny || z < 0 || z >= g.nz) continue;
    const float tw = (w0[bx] * w1[by]) * w2[bz];
    // one 16-byte load: as a vector, so that it stays one access whichever of its words the tests below need first
    const TsdfColorWords words = *reinterpret_cast<const TsdfColorWords*>(s.colors + (((size_t)z * g.ny + y) * g.nx + x));
    const TsdfColor v = {words[0], words[1], words[2], words[3]};
    const bool part = v.weight > 0.f && v.weight >= s.min_weight && tsdf_color_finite(v.b) && tsdf_color_finite(v.g) && tsdf_color_finite(v.r);
    if (!part) continue;
    den = den + tw;
    num[0] = num[0] + (tw * v.b);
    num[1] = num[1] + (tw * v.g);
    num[2] = num[2] + (tw * v.r);
  }
  if (!(den > 0.f)) return false;
  value[0] = num[0] / den, value[1] = num[1] / den, value[2] = num[2] / den;
  return true;
}

// Both outputs of pixel or point `at`; an uncoloured one gets zeros.
__host__ __device__ __forceinline__ void tsdf_color_store(const TsdfColorSampler& s, size_t at, bool colored, const float value[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = colored ? value[c] : 0.f;
    if (s.bgr_out) s.bgr_out[3 * at + c] = v;
    if (s.bgr8_out)
      s.bgr8_out[3 * at + c] = colored ? (uint8_t)__builtin_fminf(__builtin_fmaxf(__builtin_rintf(v * s.byte_scale), 0.f), 255.f) : (uint8_t)0;
  }
}

// pm_tsdf_color_map's one argument, by value.  Ri, c: the inverse of the pose (motion_inverse), as pm_tsdf_raycast carries it.
struct TsdfColorMapArgs {
  TsdfColorSampler s;
  CloudCam cam;
  double Ri[9], c[3];
  const float* disp;  // [rows][cols]
  int rows, cols;
};

// The work of one thread of k_tsdf_color_map: pixel (x, y), inside the image.  Returns whether it was coloured.
__host__ __device__ __forceinline__ bool tsdf_color_map_lane(const TsdfColorMapArgs& a, int x, int y) {
  const size_t px = (size_t)y * a.cols + x;
  const float d = a.disp[px];
  float value[3] = {0.f, 0.f, 0.f};
  bool colored = false;
  if (d > 0.f) {
    const double depth = a.cam.fxb / (double)d;
    double dx, dy, wd[3], q[3];
    tsdf_ray_direction(a.cam, a.Ri, x, y, &dx, &dy, wd);
    tsdf_ray_point(a.s.grid, a.c, wd, depth, q);
    colored = tsdf_color_sample(a.s, q, value);
  }
  tsdf_color_store(a.s, px, colored, value);
  return colored;
}

// pm_tsdf_color_points' one argument, by value.
struct TsdfColorPointsArgs {
  TsdfColorSampler s;
  const float* xyz;  // [n][3], world frame
  int n;
  const int* d_n;  // may be null: only the first min(n, *d_n) points
};

// How many points the launch works on; every lane of a wavefront reads the same word.
__host__ __device__ __forceinline__ int tsdf_color_points_limit(const TsdfColorPointsArgs& a) {
  if (!a.d_n) return a.n;
  const int m = *a.d_n;
  return m < a.n ? m : a.n;
}

// The work of one thread of k_tsdf_color_points: point `at`, in front of the limit.  Returns whether it was coloured.
__host__ __device__ __forceinline__ bool tsdf_color_point_lane(const TsdfColorPointsArgs& a, int at) {
  const TsdfGrid& g = a.s.grid;
  const float* const P = a.xyz + 3 * (size_t)at;
  const double q[3] = {((double)P[0] - g.origin[0]) / g.voxel, ((double)P[1] - g.origin[1]) / g.voxel, ((double)P[2] - g.origin[2]) / g.voxel};
  float value[3] = {0.f, 0.f, 0.f};
  const bool colored = tsdf_color_sample(a.s, q, value);
  tsdf_color_store(a.s, (size_t)at, colored, value);
  return colored;
}

}  // namespace pm
