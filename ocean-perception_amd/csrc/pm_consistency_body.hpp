// pm_consistency_body.hpp -- the per-pixel arithmetic and the per-thread body of pm_filter_consistency
// (include/pm/imaging.h), host-callable and free of kernels, so that the kernels (pm_consistency.hpp) and a CPU build
// (tests/cpp/consistency_host_main.cpp, under the sanitizers) share ONE statement of it.  The definition it is held to BIT
// FOR BIT is tests/consistency_ref.py: every operation is one rounding in the format written,
// parentheses as written (the build uses -ffp-contract=off; binary64 division and rint are IEEE on gfx950).  The projection
// of a pixel into a source is pm_reproject_disparity's own two halves (pm_reproject_body.hpp: reproject_point,
// reproject_project) with min_disp = 0 and max_disp = 0; nothing of it is restated here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_reproject_body.hpp"

namespace pm {

constexpr int kConsistencyMaxSources = PM_CONSISTENCY_MAX_SOURCES;
constexpr int kConsistencyMaxRadius = 2;
constexpr int kConsistencyLanes = kReprojectLanes;                  // a wavefront takes 64 consecutive pixels of a row ...
constexpr int kConsistencyPixelsPerLane = kReprojectPixelsPerLane;  // ... four times, 64 pixels apart (k_reproject_splat's shape)
constexpr int kConsistencyBlockX = kReprojectBlockX;                // k_consistency's block: one wavefront along a row ...
constexpr int kConsistencyBlockY = kReprojectBlockY;                // ... and rows per block; its grid is span_blocks()
constexpr int kConsistencySpan = kReprojectSpan;                    // pixels of a row per block

enum : unsigned { kConsistencyUnseen = 0, kConsistencyConsistent = 1, kConsistencyOccluded = 2, kConsistencyConflict = 3 };

// One earlier view: X_src = R X_cur + t between the left camera frames, and its map.
struct ConsistencySource {
  double R[9], t[3];
  const float* map;  // [rows][cols]
};

// The launch's one argument, by value: 8 sources of 104 bytes and 96 bytes in front of them.  The source loop indexes
// `src` with a wave-uniform index, so R, t and the map pointer are read with scalar loads.
struct ConsistencyArgs {
  CloudCam cam;
  const float* disp;
  int rows, cols;
  int n;  // sources in use, 1 .. kConsistencyMaxSources
  float max_diff;
  int min_consistent, max_conflicts;
  float* out;         // may be null, may be disp
  uint16_t* classes;  // may be null
  float* residual;    // may be null
  int* counts;        // [0] valid pixels, [1] kept pixels; zeroed
  ConsistencySource src[kConsistencyMaxSources];
};

// The class of a pixel that lands on (iu, iv) of `map` with disparity dp there (`seen`: it does land), and |e| of the
// chosen tap in *abs_e: the first tap of the (2 RADIUS + 1)^2 window, row-major, with the smallest |ds - dp| in binary64.
// Where asked for (pm_fuse_disparity, pm_fuse_body.hpp), the chosen tap's ds in *tap_ds and its index in `map` in *tap_at; 0.f
// and 0 where the class is UNSEEN.
template <int RADIUS>
__host__ __device__ __forceinline__ unsigned consistency_class(const float* map, int rows, int cols, bool seen, int iu, int iv,
                                                               float dp, double md, double* abs_e, float* tap_ds = nullptr,
                                                               size_t* tap_at = nullptr) {
  constexpr int W = 2 * RADIUS + 1;
  float ds[W * W];
#pragma unroll
  for (int dy = -RADIUS; dy <= RADIUS; ++dy)  // first every gather of the window, so that they are in flight together
#pragma unroll
    for (int dx = -RADIUS; dx <= RADIUS; ++dx) {
      const int yy = iv + dy, xx = iu + dx;
      const bool inside = seen && yy >= 0 && yy < rows && xx >= 0 && xx < cols;
      const float tap = map[inside ? (size_t)yy * cols + xx : (size_t)0];  // no branch: a tap that does not count reads pixel 0
      ds[(dy + RADIUS) * W + dx + RADIUS] = inside ? tap : 0.f;
    }
  bool found = false;
  double e = 0.0, best = 0.0;
  float chosen = 0.f;
  int at = 0;
#pragma unroll
  for (int i = 0; i < W * W; ++i) {  // then the choice, in row-major order
    const double ek = (double)ds[i] - (double)dp;
    const double ak = __builtin_fabs(ek);
    const bool take = ds[i] > 0.f && (!found || ak < best);  // a later tap replaces only with a strictly smaller |e|
    e = take ? ek : e;
    best = take ? ak : best;
    chosen = take ? ds[i] : chosen;
    at = take ? i : at;
    found = found || take;
  }
  *abs_e = best;
  if (tap_ds) *tap_ds = chosen;  // a counting tap lies inside the image: the index below is one of `map`
  if (tap_at) *tap_at = found ? (size_t)(iv + at / W - RADIUS) * cols + (iu + at % W - RADIUS) : (size_t)0;
  if (!found) return kConsistencyUnseen;
  return best <= md ? kConsistencyConsistent : e > md ? kConsistencyOccluded : kConsistencyConflict;
}

// The work of one thread of k_consistency: pixels x, x + 64, x + 128, x + 192 of row y, x < cols and y < rows.  Returns the
// thread's flags: bit k = pixel k is valid, bit 4 + k = it is kept.  The point of a pixel (three binary64 divisions) is formed
// once and kept across the sources; the four pixels give four independent binary64 chains per source.
template <int RADIUS>
__host__ __device__ __forceinline__ unsigned consistency_lane(const ConsistencyArgs& a, int x, int y) {
  constexpr int N = kConsistencyPixelsPerLane;
  const size_t row = (size_t)y * a.cols;
  float d[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int xk = x + k * kConsistencyLanes;
    d[k] = xk < a.cols ? a.disp[row + xk] : 0.f;  // the four loads are in flight together; read before any store: out may be disp
  }
  bool valid[N];
  double P[N][3], S[N];
  int n_cons[N], n_conf[N];
  unsigned cls[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    valid[k] = reproject_point(a.cam, 0.f, d[k], x + k * kConsistencyLanes, y, P[k]);
    S[k] = 0.0;
    n_cons[k] = n_conf[k] = 0;
    cls[k] = 0u;
  }
  const double md = (double)a.max_diff;
#pragma unroll 1
  for (int s = 0; s < a.n; ++s) {
    const ConsistencySource& q = a.src[s];
    int iu[N], iv[N];
    float dp[N];
    bool seen[N];
#pragma unroll
    for (int k = 0; k < N; ++k)  // four independent binary64 chains, no branch between them
      seen[k] = reproject_project(a.cam, q.R, q.t, 0.f, a.rows, a.cols, valid[k], P[k], &iu[k], &iv[k], &dp[k]);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double abs_e;
      const unsigned c = consistency_class<RADIUS>(q.map, a.rows, a.cols, seen[k], iu[k], iv[k], dp[k], md, &abs_e);
      cls[k] |= c << (2 * s);
      n_cons[k] += c == kConsistencyConsistent ? 1 : 0;
      n_conf[k] += c == kConsistencyConflict ? 1 : 0;
      S[k] = c == kConsistencyConsistent ? S[k] + abs_e : S[k];
    }
  }
  unsigned flags = 0u;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int xk = x + k * kConsistencyLanes;
    if (xk >= a.cols) continue;
    const bool kept = valid[k] && n_cons[k] >= a.min_consistent && n_conf[k] <= a.max_conflicts;
    flags |= (valid[k] ? 1u : 0u) << k | (kept ? 1u : 0u) << (4 + k);
    if (a.out) a.out[row + xk] = valid[k] && !kept ? 0.f : d[k];
    if (a.classes) a.classes[row + xk] = (uint16_t)cls[k];
    if (a.residual) a.residual[row + xk] = n_cons[k] > 0 ? (float)(S[k] / (double)(n_cons[k] > 0 ? n_cons[k] : 1)) : 0.f;
  }
  return flags;
}

}  // namespace pm
