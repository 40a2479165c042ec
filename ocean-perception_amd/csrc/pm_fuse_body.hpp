// pm_fuse_body.hpp -- the per-pixel arithmetic and the per-thread bodies of pm_fuse_disparity (include/pm/imaging.h),
// host-callable and free of kernels, so that the kernels (pm_fuse.hpp) and a CPU build (tests/cpp/fuse_host_main.cpp, under
// the sanitizers) share ONE statement of it.  The definition it is held to BIT FOR BIT is tests/fuse_ref.py (DESIGN.md section
// 8c-8): every operation is one rounding in the format written, parentheses as written (the build uses -ffp-contract=off;
// binary64 division and rint are IEEE on gfx950).  Nothing of the neighbouring stages is restated: carrying a pixel into a
// source is pm_reproject_body.hpp's reproject_point / reproject_project, the tap and the class are pm_consistency_body.hpp's
// consistency_class (which hands out the chosen tap), and a fill splat is reproject_splat_lane.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_consistency_body.hpp"

namespace pm {

constexpr int kFuseMaxSources = kConsistencyMaxSources;
constexpr int kFuseMaxRadius = kConsistencyMaxRadius;
constexpr int kFuseLanes = kConsistencyLanes;                  // a wavefront takes 64 consecutive pixels of a row ...
constexpr int kFusePixelsPerLane = kConsistencyPixelsPerLane;  // ... four times, 64 pixels apart (k_consistency's shape)
constexpr int kFuseBlockX = kConsistencyBlockX;                // the block of both kernels: one wavefront along a row ...
constexpr int kFuseBlockY = kConsistencyBlockY;                // ... and rows per block; their grid is span_blocks()
constexpr int kFuseSpan = kConsistencySpan;                    // pixels of a row per block
constexpr int kFuseCounters = 4;                               // valid, kept, fused, filled: kFusePixelsPerLane bits of fuse_lane's flags each

enum : unsigned { kFuseValid = 1, kFuseKept = 2, kFuseFused = 4, kFuseFilled = 8 };  // PM_FUSE_*

// ---- the fill splats: every source into the current view ----------------------------------------------------------------------
// One launch for all sources.  src[k]: the INVERSE of motions[k] (formed on the host in binary64) and the source's map.
struct FuseSplatArgs {
  CloudCam cam;
  int rows, cols;
  unsigned* splat;  // n maps of `px` words each, zeroed
  size_t px;
  ConsistencySource src[kFuseMaxSources];
};

// The work of one thread of k_fuse_splat for source k: reproject_splat_lane into map k.  k is wave-uniform.
__host__ __device__ __forceinline__ void fuse_splat_lane(const FuseSplatArgs& a, int k, int x, int y) {
  const ConsistencySource& q = a.src[k];
  ReprojectArgs r = {a.cam, {}, {}, 0.f, 0.f, q.map, a.rows, a.cols, a.splat + (size_t)k * a.px};
#pragma unroll
  for (int i = 0; i < 9; ++i) r.R[i] = q.R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) r.t[i] = q.t[i];
  reproject_splat_lane(r, x, y);
}

// ---- refine and fill --------------------------------------------------------------------------------------------------------
// One earlier view: X_src = R X_cur + t between the left camera frames, its map and its weights.
struct FuseSource {
  double R[9], t[3];
  const float* map;     // [rows][cols]
  const float* weight;  // [rows][cols]; null: 1.0
};

// The launch's one argument, by value: 8 sources of 112 bytes and 144 bytes in front of them.  The source loop indexes `src`
// with a wave-uniform index, so R, t and the pointers are read with scalar loads; the n splat maps are one pointer and a size.
struct FuseArgs {
  CloudCam cam;
  const float* disp;
  const float* weight;  // may be null: 1.0
  int rows, cols;
  int n;  // sources in use, 1 .. kFuseMaxSources
  float max_diff;
  int min_consistent, max_conflicts;
  int fill_min_sources;  // 0: nothing is filled and `splat` is not read
  float fill_max_diff;
  const unsigned* splat;  // k_fuse_splat's n maps of `px` words each
  size_t px;
  float* out;        // may be null, may be disp
  uint8_t* count;    // may be null
  float* spread;     // may be null
  uint8_t* flags;    // may be null
  int* counts;       // [0] valid, [1] kept, [2] fused, [3] filled pixels; zeroed
  FuseSource src[kFuseMaxSources];
};

// (double)w where w is finite and > 0, else 0: not for 0, negatives, NaN and +-inf.
__host__ __device__ __forceinline__ double fuse_weight(float w) { return w > 0.f && w < __builtin_inff() ? (double)w : 0.0; }

// The sign of a generated NaN differs between processors: a NaN result is the canonical quiet NaN.
__host__ __device__ __forceinline__ float fuse_canonical(float v) { return v != v ? __builtin_bit_cast(float, 0x7FC00000u) : v; }

// The inverse of the rigid motion X' = R X + t, formed on the host in binary64 with the parentheses as written (the build does
// not contract): what the fill splats of pm_fuse_disparity and the rays of pm_tsdf_raycast go through.
inline void motion_inverse(const double R[9], const double t[3], double Ri[9], double ti[3]) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Ri[3 * i + j] = R[3 * j + i];
    ti[i] = -(((R[i] * t[0]) + (R[3 + i] * t[1])) + (R[6 + i] * t[2]));
  }
}

// The vote of the splat maps at pixel `at`, which has no value of its own: whether it is filled, and with what.
__host__ __device__ __forceinline__ bool fuse_fill(const FuseArgs& a, size_t at, float* value, int* n_sup, float* spread) {
  unsigned m = 0u;  // the maps hold the bits of +0.0 or of a finite binary32 > 0: unsigned order is float order
#pragma unroll 1
  for (int s = 0; s < a.n; ++s) {
    const unsigned c = a.splat[(size_t)s * a.px + at];
    m = c > m ? c : m;
  }
  const double md = (double)a.fill_max_diff, mf = (double)__builtin_bit_cast(float, m);
  unsigned lo = m;
  int n = 0;
  double acc = 0.0;
#pragma unroll 1
  for (int s = 0; s < a.n; ++s) {
    const unsigned c = a.splat[(size_t)s * a.px + at];
    const double cf = (double)__builtin_bit_cast(float, c);
    const bool sup = c != 0u && __builtin_fabs(cf - mf) <= md;
    acc = sup ? acc + cf : acc;
    lo = sup && c < lo ? c : lo;
    n += sup ? 1 : 0;
  }
  const bool filled = n >= 1 && n >= a.fill_min_sources;
  *value = (float)(acc / (double)(n > 0 ? n : 1));
  *n_sup = n;
  *spread = (float)(mf - (double)__builtin_bit_cast(float, lo));
  return filled;
}

// The work of one thread of k_fuse: pixels x, x + 64, x + 128, x + 192 of row y, x < cols and y < rows.  Returns the thread's
// flags: bit k = pixel k is valid, bit 4 + k = kept, bit 8 + k = fused, bit 12 + k = filled.  The point of a pixel is formed
// once and kept across the sources, with the four accumulators of its weighted mean and spread.
template <int RADIUS>
__host__ __device__ __forceinline__ unsigned fuse_lane(const FuseArgs& a, int x, int y) {
  constexpr int N = kFusePixelsPerLane;
  const size_t row = (size_t)y * a.cols;
  float d[N], w[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int xk = x + k * kFuseLanes;
    d[k] = xk < a.cols ? a.disp[row + xk] : 0.f;  // the loads are in flight together; read before any store: out may be disp
    w[k] = a.weight && xk < a.cols ? a.weight[row + xk] : 1.f;
  }
  bool valid[N];
  double P[N][3], num[N], den[N], omin[N], omax[N];
  int n_cons[N], n_conf[N], n_obs[N], n_src[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    valid[k] = reproject_point(a.cam, 0.f, d[k], x + k * kFuseLanes, y, P[k]);
    const double w0 = fuse_weight(w[k]);
    const bool own = valid[k] && w0 > 0.0;
    num[k] = w0 * (double)d[k];
    den[k] = w0;
    omin[k] = own ? (double)d[k] : (double)__builtin_inff();
    omax[k] = own ? (double)d[k] : -(double)__builtin_inff();
    n_obs[k] = own ? 1 : 0;
    n_cons[k] = n_conf[k] = n_src[k] = 0;
  }
  const double md = (double)a.max_diff;
#pragma unroll 1
  for (int s = 0; s < a.n; ++s) {
    const FuseSource& q = a.src[s];
    int iu[N], iv[N];
    float dp[N];
    double zn[N];
    bool seen[N];
#pragma unroll
    for (int k = 0; k < N; ++k)  // four independent binary64 chains, no branch between them
      seen[k] = reproject_project(a.cam, q.R, q.t, 0.f, a.rows, a.cols, valid[k], P[k], &iu[k], &iv[k], &dp[k], &zn[k]);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double abs_e;
      float ds;
      size_t at;
      const unsigned c = consistency_class<RADIUS>(q.map, a.rows, a.cols, seen[k], iu[k], iv[k], dp[k], md, &abs_e, &ds, &at);
      const bool cons = c == kConsistencyConsistent;
      n_cons[k] += cons ? 1 : 0;
      n_conf[k] += c == kConsistencyConflict ? 1 : 0;
      const double wk = q.weight ? fuse_weight(q.weight[cons ? at : (size_t)0]) : 1.0;  // read at the chosen tap
      const double Zs = a.cam.fxb / (double)(cons ? ds : 1.f);
      const double g = zn[k] - q.t[2];
      const double Zo = ((Zs - q.t[2]) * P[k][2]) / g;  // the depth along the pixel's ray at which the source measures ds
      const double o = a.cam.fxb / Zo;
      const bool part = cons && g > 0.0 && Zo > 0.0 && __builtin_fabs(o) < (double)__builtin_inff() && wk > 0.0;
      num[k] = part ? num[k] + (wk * o) : num[k];
      den[k] = part ? den[k] + wk : den[k];
      omin[k] = part && o < omin[k] ? o : omin[k];
      omax[k] = part && o > omax[k] ? o : omax[k];
      n_obs[k] += part ? 1 : 0;
      n_src[k] += part ? 1 : 0;
    }
  }
  unsigned flags = 0u;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int xk = x + k * kFuseLanes;
    if (xk >= a.cols) continue;
    const bool kept = valid[k] && n_cons[k] >= a.min_consistent && n_conf[k] <= a.max_conflicts;
    const bool fused = kept && n_src[k] > 0;
    bool filled = false;
    float value = d[k], spread = 0.f;  // an invalid pixel that is not filled keeps its input bits
    int n_took = 0;
    if (valid[k]) {
      value = !kept ? 0.f : den[k] > 0.0 ? fuse_canonical((float)(num[k] / den[k])) : d[k];
      spread = n_obs[k] > 0 ? fuse_canonical((float)(omax[k] - omin[k])) : 0.f;
      n_took = n_obs[k];
    } else if (a.fill_min_sources >= 1) {
      float v, sp;
      int n_sup;
      filled = fuse_fill(a, row + xk, &v, &n_sup, &sp);
      value = filled ? v : value;
      spread = filled ? sp : 0.f;
      n_took = filled ? n_sup : 0;
    }
    const unsigned f = (valid[k] ? kFuseValid : 0u) | (kept ? kFuseKept : 0u) | (fused ? kFuseFused : 0u) | (filled ? kFuseFilled : 0u);
    flags |= (f & 1u) << k | ((f >> 1) & 1u) << (4 + k) | ((f >> 2) & 1u) << (8 + k) | ((f >> 3) & 1u) << (12 + k);
    if (a.out) a.out[row + xk] = value;
    if (a.count) a.count[row + xk] = (uint8_t)n_took;
    if (a.spread) a.spread[row + xk] = spread;
    if (a.flags) a.flags[row + xk] = (uint8_t)f;
  }
  return flags;
}

}  // namespace pm
