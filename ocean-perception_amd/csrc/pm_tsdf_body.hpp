// pm_tsdf_body.hpp -- the per-voxel and per-pixel arithmetic and the per-thread bodies of pm_tsdf_integrate and pm_tsdf_raycast
// (include/pm/imaging.h), host-callable and free of kernels, so that the kernels (pm_tsdf.hpp) and a CPU build
// (tests/cpp/tsdf_host_main.cpp, under the sanitizers) share ONE statement of it.  The definition it is held to BIT FOR BIT is
// tests/tsdf_ref.py: every operation is one rounding in the format written, parentheses as written
// (the build uses -ffp-contract=off; binary64 division, floor and rint are IEEE on gfx950; binary32 division and sqrt are
// correctly rounded through -fhip-fp32-correctly-rounded-divide-sqrt).  Carrying a voxel into the image is
// pm_reproject_body.hpp's reproject_project, the weight rule is pm_fuse_body.hpp's fuse_weight, the inverse pose is that
// header's motion_inverse.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_fuse_body.hpp"

namespace pm {

constexpr int kTsdfLanes = 64;  // k_tsdf_integrate: a wavefront owns 64 consecutive voxels along x; k_tsdf_raycast: 64 pixels of a row
constexpr int kTsdfWaves = 4;   // wavefronts per block of either kernel
constexpr int kTsdfBlockX = kTsdfLanes;  // the block of either kernel: threadIdx.y is the wavefront
constexpr int kTsdfBlockY = kTsdfWaves;

// One voxel: 8 bytes.  weight == 0: never observed.
struct alignas(8) TsdfVoxel {
  float tsdf, weight;
};
// Two voxels that are neighbours along x: the 16 bytes one load of a sample's corner pair fetches (8-byte aligned only).
struct alignas(8) TsdfVoxelPair {
  float tsdf0, weight0, tsdf1, weight1;
};

// pm_tsdf_volume as the launches carry it
struct TsdfGrid {
  int nx, ny, nz;
  float max_weight;
  double origin[3];
  double voxel, trunc;
};
inline TsdfGrid tsdf_grid(const pm_tsdf_volume& v) {
  return TsdfGrid{v.nx, v.ny, v.nz, v.max_weight, {v.origin[0], v.origin[1], v.origin[2]}, v.voxel, v.trunc};
}

// ---- integrate ----------------------------------------------------------------------------------------------------------------
// The launch's one argument, by value (272 bytes): the camera, the grid and the pose are wave-uniform and stay in scalar registers.
struct TsdfIntegrateArgs {
  CloudCam cam;
  TsdfGrid grid;
  double R[9], t[3];  // X_cam = R X_world + t
  float min_disp, max_range;
  const float* disp;    // [rows][cols]
  const float* weight;  // [rows][cols]; null: 1.0
  int rows, cols;
  TsdfVoxel* voxels;  // [nz][ny][nx]
  int* counts;        // [0] voxels in view, [1] voxels updated; zeroed
};

// What an updated voxel does beyond its distance record: nothing (pm_tsdf_integrate).  pm_tsdf_color_body.hpp has the other one.
struct TsdfNoColor {
  __host__ __device__ __forceinline__ unsigned operator()(size_t, size_t, double, float) const { return 0u; }
};

// The work of one thread of k_tsdf_integrate: voxel (i, j, k), inside the grid.  Returns bit 0: in view, bit 1: updated.  The
// voxel's record is touched only behind every test: a voxel outside the view or behind the band costs no volume traffic.  An
// updated voxel is handed to `more` (its number, its pixel's number, sdf, wn), whose bits are or-ed into the result: the ONE
// statement of the distance arithmetic serves pm_tsdf_integrate_color too.
template <typename More>
__host__ __device__ __forceinline__ unsigned tsdf_integrate_lane(const TsdfIntegrateArgs& a, int i, int j, int k, const More& more) {
  const TsdfGrid& g = a.grid;
  const double P[3] = {g.origin[0] + ((double)i * g.voxel), g.origin[1] + ((double)j * g.voxel), g.origin[2] + ((double)k * g.voxel)};
  int iu, iv;
  float dn;
  double Zc;
  const bool seen = reproject_project(a.cam, a.R, a.t, 0.f, a.rows, a.cols, true, P, &iu, &iv, &dn, &Zc);
  if (!seen) return 0u;
  const size_t px = (size_t)iv * a.cols + iu;
  const float d = a.disp[px];
  bool obs = d > 0.f && d >= a.min_disp;
  const double Zm = a.cam.fxb / (double)(obs ? d : 1.f);
  obs = obs && !(a.max_range != 0.f && (float)Zm > a.max_range);
  const double sdf = Zm - Zc;
  obs = obs && !(sdf < -g.trunc);
  const float f = (float)__builtin_fmin(1.0, sdf / g.trunc);
  const float wn = a.weight && obs ? a.weight[px] : 1.f;
  obs = obs && fuse_weight(wn) > 0.0;
  if (!obs) return 1u;
  const size_t voxel = ((size_t)k * g.ny + j) * g.nx + i;
  TsdfVoxel* const at = a.voxels + voxel;
  const TsdfVoxel v = *at;  // one 8-byte load ...
  TsdfVoxel o;
  o.tsdf = ((v.tsdf * v.weight) + (f * wn)) / (v.weight + wn);
  o.weight = __builtin_fminf(v.weight + wn, g.max_weight);
  *at = o;  // ... and one 8-byte store
  return 3u | more(voxel, px, sdf, wn);
}

__host__ __device__ __forceinline__ unsigned tsdf_integrate_lane(const TsdfIntegrateArgs& a, int i, int j, int k) {
  return tsdf_integrate_lane(a, i, j, k, TsdfNoColor());
}

// ---- raycast ------------------------------------------------------------------------------------------------------------------
// The launch's one argument, by value.  Ri, c: the inverse of the pose, formed on the host in binary64 (motion_inverse):
// X_world = Ri X_cam + c.
struct TsdfRaycastArgs {
  CloudCam cam;
  TsdfGrid grid;
  double R[9];  // the pose's rotation: a gradient of the grid into the camera frame
  double Ri[9], c[3];
  double min_range, max_range;  // (double) of the options' floats
  double ds;                    // (double)step * trunc
  float min_weight;
  int n_samples;  // the n with min_range + ((double)n * ds) <= max_range: 0 .. n_samples - 1, counted on the host
  const TsdfVoxel* voxels;
  int rows, cols;
  float* disp_out;     // [rows][cols]; may be null
  float* normals_out;  // [rows][cols][3]; may be null
  int* counts;         // [0] pixels hit; zeroed
};

// The number of samples of a ray (host only): the n >= 0 with lo + ((double)n * ds) <= hi, decided by that very expression; -1
// where ds is not > 0 or there are more than kTsdfMaxSamples of them.
constexpr int kTsdfMaxSamples = 1 << 16;
inline int tsdf_sample_count(double lo, double hi, double ds) {
  const double estimate = (hi - lo) / ds;
  if (!(ds > 0.0) || !(estimate >= 0.0) || !(estimate < (double)kTsdfMaxSamples - 2.0)) return -1;
  int n = (int)estimate + 1;
  while (lo + ((double)n * ds) <= hi) ++n;
  while (n > 0 && !(lo + ((double)(n - 1) * ds) <= hi)) --n;
  return n;
}

__host__ __device__ __forceinline__ float tsdf_lerp(float a, float b, float t) { return a + (t * (b - a)); }

// The trilinear value of the volume at grid coordinates q (voxel (0, 0, 0)'s centre is (0, 0, 0)); false where one of the eight
// corners lies outside the grid or takes no part (weight > 0 && weight >= min_weight).  The corners of a sample are four
// 16-byte loads: (b0, b0 + 1) are neighbours in memory.
__host__ __device__ __forceinline__ bool tsdf_sample(const TsdfGrid& g, const TsdfVoxel* voxels, float min_weight, const double q[3],
                                                     float* value) {
  const double b0 = __builtin_floor(q[0]), b1 = __builtin_floor(q[1]), b2 = __builtin_floor(q[2]);
  const float f0 = (float)(q[0] - b0), f1 = (float)(q[1] - b1), f2 = (float)(q[2] - b2);
  // NaN fails every comparison; b + 1 <= n - 1 in binary64, so nothing is converted before it is known to fit
  const bool inside = b0 >= 0.0 && b0 <= (double)g.nx - 2.0 && b1 >= 0.0 && b1 <= (double)g.ny - 2.0 && b2 >= 0.0 && b2 <= (double)g.nz - 2.0;
  if (!inside) return false;
  const size_t sx = 1, sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny;
  const size_t at = ((size_t)(int)b2 * sz + (size_t)(int)b1 * sy) + (size_t)(int)b0 * sx;
  TsdfVoxelPair p00, p10, p01, p11;  // p<dy><dz>: corners (0, dy, dz) and (1, dy, dz)
  __builtin_memcpy(&p00, voxels + at, sizeof p00);
  __builtin_memcpy(&p10, voxels + at + sy, sizeof p10);
  __builtin_memcpy(&p01, voxels + at + sz, sizeof p01);
  __builtin_memcpy(&p11, voxels + at + sz + sy, sizeof p11);
  const float mw = min_weight;
  const bool part = p00.weight0 > 0.f && p00.weight0 >= mw && p00.weight1 > 0.f && p00.weight1 >= mw &&
                    p10.weight0 > 0.f && p10.weight0 >= mw && p10.weight1 > 0.f && p10.weight1 >= mw &&
                    p01.weight0 > 0.f && p01.weight0 >= mw && p01.weight1 > 0.f && p01.weight1 >= mw &&
                    p11.weight0 > 0.f && p11.weight0 >= mw && p11.weight1 > 0.f && p11.weight1 >= mw;
  const float x00 = tsdf_lerp(p00.tsdf0, p00.tsdf1, f0);
  const float x10 = tsdf_lerp(p10.tsdf0, p10.tsdf1, f0);
  const float x01 = tsdf_lerp(p01.tsdf0, p01.tsdf1, f0);
  const float x11 = tsdf_lerp(p11.tsdf0, p11.tsdf1, f0);
  const float y0 = tsdf_lerp(x00, x10, f1);
  const float y1 = tsdf_lerp(x01, x11, f1);
  *value = tsdf_lerp(y0, y1, f2);
  return part;
}

// The grid coordinates of the point at depth s along the ray from c whose direction in the world frame is wd.
__host__ __device__ __forceinline__ void tsdf_ray_point(const TsdfGrid& g, const double c[3], const double wd[3], double s, double q[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) q[i] = ((c[i] + (s * wd[i])) - g.origin[i]) / g.voxel;
}
__host__ __device__ __forceinline__ void tsdf_ray_point(const TsdfRaycastArgs& a, const double wd[3], double s, double q[3]) {
  tsdf_ray_point(a.grid, a.c, wd, s, q);
}

// The ray of pixel (x, y): (dx, dy, 1) in the camera frame, wd in the world frame (Ri: the inverse pose's rotation).
__host__ __device__ __forceinline__ void tsdf_ray_direction(const CloudCam& cam, const double Ri[9], int x, int y, double* dx, double* dy,
                                                            double wd[3]) {
  *dx = ((double)x - cam.cx) / cam.fx, *dy = ((double)y - cam.cy) / cam.fy;
#pragma unroll
  for (int i = 0; i < 3; ++i) wd[i] = ((Ri[3 * i] * *dx) + (Ri[3 * i + 1] * *dy)) + Ri[3 * i + 2];
}

// The work of one thread of k_tsdf_raycast: pixel (x, y), inside the image.  Returns whether the ray hit.  The ray in the camera
// frame is (dx, dy, 1), so the ray parameter is the camera depth; no operation divides by a component of the direction.
__host__ __device__ __forceinline__ bool tsdf_ray_lane(const TsdfRaycastArgs& a, int x, int y) {
  double dx, dy, wd[3];
  tsdf_ray_direction(a.cam, a.Ri, x, y, &dx, &dy, wd);
  bool have_prev = false, hit = false;
  float f_prev = 0.f;
  double s_hit = 1.0;
#pragma unroll 1
  for (int n = 0; n < a.n_samples; ++n) {
    const double s = a.min_range + ((double)n * a.ds);  // never accumulated
    double q[3];
    tsdf_ray_point(a, wd, s, q);
    float f_cur = 0.f;
    const bool valid = tsdf_sample(a.grid, a.voxels, a.min_weight, q, &f_cur);
    if (valid && have_prev && f_prev > 0.f && f_cur <= 0.f) {
      const double s_prev = a.min_range + ((double)(n - 1) * a.ds);
      s_hit = s_prev + (a.ds * ((double)f_prev / ((double)f_prev - (double)f_cur)));
      hit = true;
      break;
    }
    if (valid && have_prev && f_prev < 0.f && f_cur > 0.f) break;  // a back face ends the ray
    have_prev = valid;  // an invalid sample forgets f_prev
    f_prev = f_cur;
  }
  const size_t px = (size_t)y * a.cols + x;
  if (a.disp_out) a.disp_out[px] = hit ? (float)(a.cam.fxb / s_hit) : 0.f;
  if (a.normals_out) {
    float nrm[3] = {0.f, 0.f, 0.f};
    if (hit) {
      double q[3];
      tsdf_ray_point(a, wd, s_hit, q);
      float grad[3];
      bool all = true;
#pragma unroll
      for (int i = 0; i < 3; ++i) {  // central differences one voxel either side, along the grid's axes
        double qp[3] = {q[0], q[1], q[2]}, qm[3] = {q[0], q[1], q[2]};
        qp[i] = q[i] + 1.0;
        qm[i] = q[i] - 1.0;
        float vp = 0.f, vm = 0.f;
        const bool okp = tsdf_sample(a.grid, a.voxels, a.min_weight, qp, &vp);
        const bool okm = tsdf_sample(a.grid, a.voxels, a.min_weight, qm, &vm);
        all = all && okp && okm;
        grad[i] = vp - vm;
      }
      const double g0 = (double)grad[0], g1 = (double)grad[1], g2 = (double)grad[2];
      double m[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) m[i] = ((a.R[3 * i] * g0) + (a.R[3 * i + 1] * g1)) + (a.R[3 * i + 2] * g2);
      const float nx = (float)m[0], ny = (float)m[1], nz = (float)m[2];
      const float s = ((nx * nx) + (ny * ny)) + (nz * nz);  // pm_planes_normals' normalisation (cloud_normal)
      const float l = __builtin_sqrtf(s);
      const bool ok = all && l > 0.f && l < __builtin_inff();
      const float q1 = ok ? l : 1.f;
      const bool away = (((m[0] * dx) + (m[1] * dy)) + m[2]) > 0.0;  // along the ray: turned to face the camera
      nrm[0] = !ok ? 0.f : away ? -(nx / q1) : nx / q1;
      nrm[1] = !ok ? 0.f : away ? -(ny / q1) : ny / q1;
      nrm[2] = !ok ? 0.f : away ? -(nz / q1) : nz / q1;
    }
    float* o = a.normals_out + px * 3;
    o[0] = nrm[0], o[1] = nrm[1], o[2] = nrm[2];
  }
  return hit;
}

}  // namespace pm
