// pm_confidence_body.hpp -- the per-pixel arithmetic and the per-thread steps of pm_disparity_confidence
// (include/pm/imaging.h), host-callable and free of kernels, so that the kernels (pm_confidence.hpp) and a CPU build
// (tests/cpp/confidence_host_main.cpp, under the sanitizers) share ONE statement of them.  The definition they are held to
// BIT FOR BIT is tests/confidence_ref.py.  A cost is the engine's own: cpu_lerp, cpu_tap_color,
// cpu_tap_grad and cpu_cost_from_sums of pm_device.hpp, nothing of them is restated here; the build uses -ffp-contract=off.
//
// A workgroup's work comes as the steps its threads take between barriers -- confidence_lane_setup, confidence_fill,
// confidence_lane_finish -- so that a host can walk a block thread by thread over exactly sized stand-ins for the LDS tile.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm/imaging.h"
#include "pm_device.hpp"
#include "pm_reproject_body.hpp"  // reproject_add

namespace pm {

constexpr int kConfTileW = 32, kConfTileH = 8;  // pixels of a workgroup, one per thread
constexpr int kConfThreads = kConfTileW * kConfTileH;
constexpr int kConfTileRW = 224;  // columns of the target tile held in LDS

// The launch's one argument, by value.
struct ConfidenceArgs {
  const uint8_t* left;   // [rows][cols], packed
  const uint8_t* right;
  const uint8_t* gl8;    // scratch: sat_u8 of the left image's Sobel magnitude (what a window reads of its own image)
  const float* gr;       // scratch: the right image's Sobel magnitude
  const float* disp_l;
  const float* disp_r;   // may be null
  int rows, cols, pw, ph;
  float max_cost, min_margin, min_bg_margin, max_lr_diff;
  int drop_unmeasured;
  CostParams cp;         // the PM_SEM_CPU functor of the handle for this window
  float* out;            // may be null, may be disp_l
  float* measures;       // [4][rows][cols], may be null
  uint8_t* flags;        // may be null
  int* counts;           // [0] valid, [1] measured, [2] kept; zeroed
};

// The PM_SEM_CPU functor (alpha, tau_color, tau_grad) over a pw x ph window as the cost arithmetic takes it.
inline CostParams confidence_cost_params(float alpha, float tau_color, float tau_grad, int pw, int ph) {
  CostParams cp = {};
  cp.semantics = 0;  // PM_SEM_CPU
  cp.pw = pw, cp.ph = ph;
  cp.alpha = alpha, cp.one_minus_alpha = 1.f - alpha, cp.tau_color = tau_color, cp.tau_grad = tau_grad;
  cp.inv_n = 1. / (double)(pw * ph);
  cp.inv_n_hi = (float)cp.inv_n, cp.inv_n_lo = (float)(cp.inv_n - (double)cp.inv_n_hi);
  return cp;
}

// The LDS tile of a workgroup (or a host's stand-in for it): the reference window rows of the 32x8 pixels and the target rows
// over the columns lo4 .. lo4 + rw - 1, both over the image rows y0 - ph / 2 .. y0 + 7 + ph / 2, rows and columns clamped
// into the image.
struct ConfidenceTile {
  uint8_t* l8;   // [tr][lwp]          left image, columns x0 - pw / 2 ..
  uint8_t* lg;   // [tr][lwp]          its saturated gradient
  uint8_t* r8;   // [tr][kConfTileRW]  right image
  uint8_t* rg8;  // [tr][kConfTileRW]  sat_u8 of its gradient: the d = 0 sample
  float* rg;     // [tr][kConfTileRW]  its gradient
  int lwp;       // row stride of the reference tiles
  int lo4, rw;   // first column and width of the target tile
};
__host__ __device__ __forceinline__ int confidence_tile_rows(int ph) { return kConfTileH + ph - 1; }
__host__ __device__ __forceinline__ int confidence_tile_lwp(int pw) { return (kConfTileW + pw - 1 + 3) & ~3; }

// What a thread knows of its pixel before the block's barrier.
struct ConfidenceLane {
  float d;
  bool valid, measured, has_m, has_p;
  float dm, dp;
  int lo, hi;  // target columns this pixel's four windows start at: smallest and largest ipx (measured pixels only)
};

__host__ __device__ __forceinline__ ConfidenceLane confidence_lane_setup(const ConfidenceArgs& a, int x, int y) {
  ConfidenceLane l = {};
  if (x >= a.cols || y >= a.rows) return l;
  l.d = a.disp_l[(size_t)y * a.cols + x];  // read before any store: out may be disp_l
  l.valid = l.d > 0.f;
  const bool interior = x >= a.pw / 2 && x <= a.cols - a.pw / 2 - 1 && y >= a.ph / 2 && y <= a.rows - a.ph / 2 - 1;
  const float hi = (float)x - (float)(a.pw / 2);
  l.measured = l.valid && interior && l.d <= hi;
  l.dm = l.d - 1.0f;
  l.dp = l.d + 1.0f;
  l.has_m = l.measured && l.dm >= 0.f;
  l.has_p = l.measured && l.dp <= hi;
  if (l.measured) {
    l.lo = cpu_lerp(x, l.has_p ? l.dp : l.d, a.pw).ipx;  // ipx does not grow with d
    l.hi = x - a.pw / 2;                                 // cost(0)
  }
  return l;
}

// Thread `tid`'s share of the tile fill: wavefront w takes the tile rows w, w + 4, ..., its lanes the columns 64 apart.
__host__ __device__ __forceinline__ void confidence_fill(const ConfidenceArgs& a, const ConfidenceTile& t, int x0, int y0, int tid) {
  const int fw = tid >> 6, fl = tid & 63;
  const int tr = confidence_tile_rows(a.ph), lw = kConfTileW + a.pw - 1;
  const int ry0 = y0 - a.ph / 2, lx0 = x0 - a.pw / 2;
  for (int rr = fw; rr < tr; rr += 4) {
    int gy = ry0 + rr;
    gy = gy < 0 ? 0 : gy > a.rows - 1 ? a.rows - 1 : gy;
    const size_t row = (size_t)gy * a.cols;
    for (int cc = fl; cc < lw; cc += 64) {
      int gx = lx0 + cc;
      gx = gx < 0 ? 0 : gx > a.cols - 1 ? a.cols - 1 : gx;
      t.l8[rr * t.lwp + cc] = a.left[row + gx];
      t.lg[rr * t.lwp + cc] = a.gl8[row + gx];
    }
    for (int cc = fl; cc < t.rw; cc += 64) {
      int gx = t.lo4 + cc;
      gx = gx < 0 ? 0 : gx > a.cols - 1 ? a.cols - 1 : gx;
      const float g = a.gr[row + gx];
      t.r8[rr * kConfTileRW + cc] = a.right[row + gx];
      t.rg[rr * kConfTileRW + cc] = g;
      t.rg8[rr * kConfTileRW + cc] = (uint8_t)sat_u8(g);
    }
  }
}

// Where a pixel's windows are read from.  Window row i of the reference starts at ref8(i) / refg8(i); target column c of
// that row is tgt8(i)[c - cbase] and tgtg(i)[c - cbase].
struct ConfidenceGlobalSrc {
  const ConfidenceArgs& a;
  int x, y;
  static constexpr bool kHasG8 = false;
  __host__ __device__ __forceinline__ size_t row(int i) const { return (size_t)(y - a.ph / 2 + i) * a.cols; }
  __host__ __device__ __forceinline__ const uint8_t* ref8(int i) const { return a.left + row(i) + (x - a.pw / 2); }
  __host__ __device__ __forceinline__ const uint8_t* refg8(int i) const { return a.gl8 + row(i) + (x - a.pw / 2); }
  __host__ __device__ __forceinline__ const uint8_t* tgt8(int i) const { return a.right + row(i); }
  __host__ __device__ __forceinline__ const float* tgtg(int i) const { return a.gr + row(i); }
  __host__ __device__ __forceinline__ const uint8_t* tgtg8(int) const { return nullptr; }
  __host__ __device__ __forceinline__ int cbase() const { return 0; }
};
struct ConfidenceTileSrc {
  const ConfidenceTile& t;
  int tx, ty;
  static constexpr bool kHasG8 = true;
  __host__ __device__ __forceinline__ const uint8_t* ref8(int i) const { return t.l8 + (ty + i) * t.lwp + tx; }
  __host__ __device__ __forceinline__ const uint8_t* refg8(int i) const { return t.lg + (ty + i) * t.lwp + tx; }
  __host__ __device__ __forceinline__ const uint8_t* tgt8(int i) const { return t.r8 + (ty + i) * kConfTileRW; }
  __host__ __device__ __forceinline__ const float* tgtg(int i) const { return t.rg + (ty + i) * kConfTileRW; }
  __host__ __device__ __forceinline__ const uint8_t* tgtg8(int i) const { return t.rg8 + (ty + i) * kConfTileRW; }
  __host__ __device__ __forceinline__ int cbase() const { return t.lo4; }
};

// The background sample of target column c of window row i -- cost(+0.0f): the fraction is 0, so the colour sample is the
// target byte itself and the gradient sample its saturated gradient, a plain byte SAD (k_background_tiled).  A source without
// the saturated plane rounds the gradient here.
template <typename Src>
__host__ __device__ __forceinline__ unsigned confidence_bg_grad(const Src& s, int i, int c) {
  if constexpr (Src::kHasG8)
    return s.tgtg8(i)[c];
  else
    return sat_u8_pk(s.tgtg(i)[c]);
}

// cost(d) of one window, cpu_cost_lane's loop (pm_device.hpp) over a source, with the one-instruction accumulate forms
// (cpu_acc_color, cpu_acc_grad): PW, PH > 0 unroll a row.  BG: cost(+0.0f) of pixel x as well, in *c_bg, from the same pass
// over the reference bytes.
template <int PW, int PH, bool BG, typename Src>
__host__ __device__ __forceinline__ float confidence_cost(const ConfidenceArgs& a, const Src& s, const CpuLerp& l, int x, float* c_bg) {
  const int pw = PW ? PW : a.pw, ph = PH ? PH : a.ph, cb = s.cbase(), cz = x - pw / 2 - cb;
  unsigned sc = 0, sg = 0, bc = 0, bg = 0;
#pragma unroll 1
  for (int i = 0; i < ph; ++i) {
    const uint8_t* lp = s.ref8(i);
    const uint8_t* lg = s.refg8(i);
    const uint8_t* rp = s.tgt8(i);
    const float* rg = s.tgtg(i);
    int c0 = l.ipx;
    int r0 = rp[c0 - cb];
    float g0 = rg[c0 - cb];
#pragma unroll
    for (int j = 0; j < pw; ++j) {
      const int c1 = c0 + 1 < a.cols ? c0 + 1 : a.cols - 1;
      const int r1 = rp[c1 - cb];
      const float g1 = rg[c1 - cb];
      const int pl = lp[j], pg = lg[j];
      sc = cpu_acc_color(sc, pl, r0, r1, l);
      sg = cpu_acc_grad(sg, pg, g0, g1, l);
      if (BG) {
        bc = sad_u8((unsigned)pl, rp[cz + j], bc);
        bg = sad_u8((unsigned)pg, confidence_bg_grad(s, i, cz + j), bg);
      }
      r0 = r1;
      g0 = g1;
      c0 = c1;
    }
  }
  if (BG) *c_bg = cpu_cost_from_sums((int)bc, (int)bg, a.cp);
  return cpu_cost_from_sums((int)sc, (int)sg, a.cp);
}

// cost(d + 1), cost(d), cost(d - 1) where the three windows are one apart and share their fraction (l is cost(d + 1)'s lerp,
// its ipx >= 0 and ipx + pw + 2 <= cols + 1): ONE pass over the pw + 2 lerped columns of a row serves all three, and
// cost(+0.0f) of pixel x (*c_bg) rides on its reference bytes; every sample is formed exactly as confidence_cost forms it.
template <int PW, int PH, typename Src>
__host__ __device__ __forceinline__ void confidence_cost3(const ConfidenceArgs& a, const Src& s, const CpuLerp& l, int x, float* cp_,
                                                          float* c0_, float* cm_, float* c_bg) {
  const int pw = PW ? PW : a.pw, ph = PH ? PH : a.ph, cb = s.cbase(), cz = x - pw / 2 - cb;
  unsigned sc0 = 0, sc1 = 0, sc2 = 0, sg0 = 0, sg1 = 0, sg2 = 0, bc = 0, bg = 0;  // window 0: d + 1, 1: d, 2: d - 1
#pragma unroll 1
  for (int i = 0; i < ph; ++i) {
    const uint8_t* lp = s.ref8(i);
    const uint8_t* lg = s.refg8(i);
    const uint8_t* rp = s.tgt8(i);
    const float* rg = s.tgtg(i);
    int c0 = l.ipx;
    int r0 = rp[c0 - cb];
    float g0 = rg[c0 - cb];
#pragma unroll
    for (int j = 0; j < pw + 2; ++j) {
      const int c1 = c0 + 1 < a.cols ? c0 + 1 : a.cols - 1;
      const int r1 = rp[c1 - cb];
      const float g1 = rg[c1 - cb];
      if (j < pw) {  // sample j is tap j - k of window k
        const int pl = lp[j], pg = lg[j];
        sc0 = cpu_acc_color(sc0, pl, r0, r1, l);
        sg0 = cpu_acc_grad(sg0, pg, g0, g1, l);
        bc = sad_u8((unsigned)pl, rp[cz + j], bc);
        bg = sad_u8((unsigned)pg, confidence_bg_grad(s, i, cz + j), bg);
      }
      if (j >= 1 && j <= pw) {
        sc1 = cpu_acc_color(sc1, lp[j - 1], r0, r1, l);
        sg1 = cpu_acc_grad(sg1, lg[j - 1], g0, g1, l);
      }
      if (j >= 2) {
        sc2 = cpu_acc_color(sc2, lp[j - 2], r0, r1, l);
        sg2 = cpu_acc_grad(sg2, lg[j - 2], g0, g1, l);
      }
      r0 = r1;
      g0 = g1;
      c0 = c1;
    }
  }
  *cp_ = cpu_cost_from_sums((int)sc0, (int)sg0, a.cp);
  *c0_ = cpu_cost_from_sums((int)sc1, (int)sg1, a.cp);
  *cm_ = cpu_cost_from_sums((int)sc2, (int)sg2, a.cp);
  *c_bg = cpu_cost_from_sums((int)bc, (int)bg, a.cp);
}

// The four measures and the verdicts of a measured pixel, and every store of a pixel inside the image.  Returns the
// pixel's count bits: 1 valid, 2 measured, 4 kept.
template <int PW, int PH, typename Src>
__host__ __device__ __forceinline__ unsigned confidence_lane_finish(const ConfidenceArgs& a, const ConfidenceLane& l, const Src& s,
                                                                    int x, int y) {
  const int pw = PW ? PW : a.pw;
  const float inf = __builtin_huge_valf();
  float c0 = -1.0f, margin = 0.f, bg_margin = 0.f, lr = inf;
  unsigned flags = 0u;
  if (l.measured) {
    const CpuLerp l0 = cpu_lerp(x, l.d, pw);
    float cm = 0.f, cp = 0.f, c_bg = 0.f;
    bool together = false;
    if (l.has_m && l.has_p) {
      const CpuLerp lm = cpu_lerp(x, l.dm, pw), lp = cpu_lerp(x, l.dp, pw);
      together = lm.a == l0.a && lp.a == l0.a && lm.ipx == l0.ipx + 1 && lp.ipx == l0.ipx - 1;
    }
    if (together) {
      confidence_cost3<PW, PH>(a, s, cpu_lerp(x, l.dp, pw), x, &cp, &c0, &cm, &c_bg);
    } else {  // each on its own
      c0 = confidence_cost<PW, PH, true>(a, s, l0, x, &c_bg);
#pragma unroll 1
      for (int k = 1; k < 3; ++k) {  // ONE copy of this window loop in the code, no array of lerps
        if ((k == 1 && !l.has_m) || (k == 2 && !l.has_p)) continue;
        // d - 1.0f, d + 1.0f: one addition each, as the definition forms them; picking l.dm / l.dp by k would index memory
        const float c = confidence_cost<PW, PH, false>(a, s, cpu_lerp(x, l.d + (k == 1 ? -1.0f : 1.0f), pw), x, nullptr);
        cm = k == 1 ? c : cm;
        cp = k == 2 ? c : cp;
      }
    }
    if (l.has_m && l.has_p) {
      const float cn = cp < cm ? cp : cm;
      margin = cn - c0;
    } else if (l.has_m) {
      margin = cm - c0;
    } else if (l.has_p) {
      margin = cp - c0;
    }
    bg_margin = c_bg - c0;
    flags = PM_CONF_MEASURED;
    if (a.disp_r) {
      const int q = (int)fmaxf((float)x - l.d, 0.f);  // pm_mask_occlusions' index: pw / 2 <= q <= x here
      const float r = a.disp_r[(size_t)y * a.cols + q];
      if (r > 0.f) lr = (float)__builtin_fabs((double)r - (double)l.d);
      if (!(lr <= a.max_lr_diff)) flags |= PM_CONF_FAIL_LR;
    }
    if (!(c0 <= a.max_cost)) flags |= PM_CONF_FAIL_COST;
    if (!(margin >= a.min_margin)) flags |= PM_CONF_FAIL_MARGIN;
    if (!(bg_margin >= a.min_bg_margin)) flags |= PM_CONF_FAIL_BG;
  }
  const bool kept = flags == PM_CONF_MEASURED;
  if (x < a.cols && y < a.rows) {
    const size_t o = (size_t)y * a.cols + x, plane = (size_t)a.rows * a.cols;
    if (a.out) a.out[o] = (l.measured && !kept) || (a.drop_unmeasured && l.valid && !l.measured) ? 0.f : l.d;
    if (a.measures) {
      a.measures[o] = c0;
      a.measures[plane + o] = margin;
      a.measures[2 * plane + o] = bg_margin;
      a.measures[3 * plane + o] = lr;
    }
    if (a.flags) a.flags[o] = (uint8_t)flags;
  }
  return (l.valid ? 1u : 0u) | (l.measured ? 2u : 0u) | (kept ? 4u : 0u);
}

// The target tile of a block whose measured pixels' windows start at columns lo .. hi: it begins at the multiple of four
// below lo and ends behind the second tap of the last window column.  False: the span exceeds what the LDS holds.
__host__ __device__ __forceinline__ bool confidence_tile_plan(int lo, int hi, int pw, int* lo4, int* rw) {
  *lo4 = lo & ~3;
  *rw = hi + pw + 1 - *lo4;
  return *rw <= kConfTileRW;
}

}  // namespace pm
