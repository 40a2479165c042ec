// pm_planes_plan.hpp -- what a launch of the plane-mode kernel (pm_planes.hpp::k_planes) is made of: ONE pure host
// function, plan_planes.  pl_launch_w takes its grid and its dynamic LDS from the result, pm_debug_planes_plan
// (include/pm/testing.h) returns it without a device, pm_debug_planes_last returns what a handle's last stage launched,
// tests/test_plane_stages.py pins it.  No HIP header: this compiles with a host compiler alone
// (tests/cpp/planes_plan_main.cpp).  No choice made here changes a result.
// What the kernel and the plan must agree on lives here once: the tile sizes, the dwords of a reference row, the order in
// which a checkerboard row pair's taps are grouped (PlPairOrder) and the predicate of the fast target-tile fill.
#pragma once

#include <cstddef>

#include "pm_sweep_defs.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PM_PL_HD __host__ __device__
#else
#define PM_PL_HD
#endif

namespace pm {

enum { PL_INIT = 0, PL_SPATIAL = 1, PL_VIEW = 2, PL_REFINE = 3, PL_VIEW_REFINE = 4 };  // 4 = 2 then 3, one tile fill

// Tile height (rows = wavefronts of a block) per stage.  Results do not depend on it; what it trades is the halo (P - 1
// extra rows of reference and target tile per block), the wavefronts a CU holds, and how evenly a launch's blocks fill
// the chip's block slots (a 1280x720 view is 1800 blocks of 8 rows: 2.3 rounds on the 768 slots three blocks per CU give).
// -DPL_TILE_H_SPATIAL / -DPL_TILE_H_OTHER: A/B builds (profiles/r06_planes_tile_height.txt).
#ifndef PL_TILE_H_SPATIAL
#define PL_TILE_H_SPATIAL 8
#endif
#ifndef PL_TILE_H_OTHER
#define PL_TILE_H_OTHER 8
#endif
#ifndef PL_SPATIAL_REF_REGS
#define PL_SPATIAL_REF_REGS 1
#endif
PM_PL_HD constexpr int pl_tile_h(int stage) { return stage == PL_SPATIAL ? PL_TILE_H_SPATIAL : PL_TILE_H_OTHER; }

// Tile width.  The spatial stage updates one colour: 64 active lanes per row of a 128-wide tile.  The other stages update
// every pixel: 64-wide tiles, one pixel per lane.  -DPL_WIDE_TW=128 gives them 128-wide tiles whose lanes take two pixels
// of a row one after the other (half as many blocks per launch, the 164 extra target columns of a tile row amortised
// over 128 pixels); tried for the last, partly filled round of blocks of a launch (900 blocks on 512 slots instead of
// 1800 on 768) and dropped: 241 -> 231 pairs/s -- two blocks per CU instead of three leave 4 wavefronts per SIMD
// instead of 6, which costs more than the tail gains (bit-identical either way).
#ifndef PL_WIDE_TW
#define PL_WIDE_TW 64
#endif
PM_PL_HD constexpr int pl_tile_w(int stage) { return stage == PL_SPATIAL ? 128 : PL_WIDE_TW; }
PM_PL_HD constexpr int pl_ref_row_dwords(int LW, int win) {
  // dwords per reference row (+1: a shifted copy reads 3 bytes further); checkerboard: per column-parity half
  return win == 1 ? ((LW + 1) / 2 + 3) / 4 + 1 : (LW + 3) / 4 + 1;
}

struct PlanesParams {
  int patch, max_disp, refine_steps, margin;
  float slope_max;  // effective bound (f16-representable in f16 mode)
  float slope_init, slope_per_disp;
  float alpha, one_minus_alpha, tau_color, tau_grad, inv_n;
  float lr_tol;
  unsigned long long seed;
  int n_views;
  int window;  // PM_PL_WINDOW_FULL / PM_PL_WINDOW_CHECKER (pm/patchmatch.h): which taps of the P x P window count
  int neighbours;  // PM_PL_NEIGH_FOUR / PM_PL_NEIGH_TWO: the spatial stage's candidates
};

// Target columns a tile row holds: the tile, the window on either side, every admissible disparity to the left, the
// slope margin on either side, and the right neighbour of the last tap.
PM_PL_HD constexpr int pl_target_row_entries(int TW, int P, int max_disp, int margin) {
  return TW + 2 * (P / 2) + max_disp + 2 * margin + 2;
}

// The fast fill of the target tile: one dword (two pixels) per lane, row and 128-column strip, the loads of up to
// kPlFillStrips strips in flight together.  It needs rows of whole dwords -- an even `cols` and a target plane that
// starts on a 4-byte boundary (tgt_aligned4) -- and a tile row of at most 128 * kPlFillStrips entries beside the one
// column the even start may add; every other launch fills entry by entry.  k_planes and plan_planes both decide here.
constexpr int kPlFillStrips = 4;
PM_PL_HD constexpr bool pl_fast_fill(int cols, int rw, bool tgt_aligned4) {
  return (cols & 1) == 0 && tgt_aligned4 && rw + 1 <= 128 * kPlFillStrips;
}

// Two window rows of the checkerboard at once (round 6): an even row has NE = (P + 1) / 2 taps, the odd row behind it
// NO = P / 2 -- 6 and 5 for P = 11 -- so both end in a partial group of four (2 taps and 1 tap), and a partial group costs
// what a full one does (byte gathers, two v_sad_u8, masks).  Where the two leftovers fit ONE group they share it: the
// samples are taken in the order [even full groups | odd full groups | even leftover, odd leftover], the reference bytes of
// the shared group come from one v_perm_b32 of the two rows' last dwords (zero where the group is short: no masks).
// P = 11: 3 groups per row pair instead of 4, 20 vector instructions for gathers and SADs instead of 26.
template <int P>
struct PlPairOrder {
  static constexpr int NE = (P + 1) / 2, NO = P / 2, QE = NE / 4, QO = NO / 4, RE = NE % 4, RO = NO % 4, NT = NE + NO;
  static constexpr bool shared = RE > 0 && RO > 0 && RE + RO <= 4;
  int odd[NT], idx[NT];
  constexpr PlPairOrder() : odd{}, idx{} {
    int k = 0;
    for (int j = 0; j < 4 * QE; ++j, ++k) { odd[k] = 0; idx[k] = j; }
    for (int j = 0; j < 4 * QO; ++j, ++k) { odd[k] = 1; idx[k] = j; }
    for (int j = 4 * QE; j < NE; ++j, ++k) { odd[k] = 0; idx[k] = j; }
    for (int j = 4 * QO; j < NO; ++j, ++k) { odd[k] = 1; idx[k] = j; }
  }
  // v_perm_b32 selector of the shared group's reference bytes: RE bytes of the even row's last dword (source 1: bytes
  // 0..3), then RO bytes of the odd row's (source 0: bytes 4..7), then zeros (0x0c)
  static constexpr unsigned sel() {
    unsigned v = 0;
    for (int b = 0; b < 4; ++b) {
      const unsigned s = b < RE ? (unsigned)b : (b < RE + RO ? (unsigned)(4 + b - RE) : 0x0cu);
      v |= s << (8 * b);
    }
    return v;
  }
};

// What plan_planes decided for one launch of k_planes<P, stage, state type, window shape>.  Host-side only.
struct PlanesVariant {
  int launched = 0;    // 1: a kernel runs; 0: the stage is a no-op for these parameters, and everything else is 0
  int stage = 0;       // PL_*: the instantiation that runs (PL_VIEW_REFINE with one view runs PL_REFINE)
  int patch = 0;       // window P
  int window = 0;      // PM_PL_WINDOW_FULL / PM_PL_WINDOW_CHECKER
  int state_f16 = 0;   // 0: f32 state, 1: f16
  int tile_w = 0, tile_h = 0;
  int grid_x = 0, grid_y = 0;
  int lds_bytes = 0;   // dynamic LDS of the launch
  int rw = 0;          // entries of a target tile row
  int margin = 0;      // PlanesParams::margin
  int fast_fill = 0;   // 1: pl_fast_fill holds
  int ref_regs = 0;    // 1: the spatial stage keeps the reference window in registers (checkerboard, shared leftover group)
  int tap_class = 0;   // how the window's taps are grouped by fours, see pl_tap_class
};

// One id per distinct grouping of a window's leftover taps.  Checkerboard: 4 * RE + RO of PlPairOrder<P> -- the taps an
// even and an odd window row leave beyond their whole groups of four (9 for P = 3 and 11, which share one group, 14 for
// 5 and 13, 3 for 7 and 15, 4 for 9).  Full window: 16 + P % 4, the taps of a row beyond its whole groups.
template <int P>
constexpr int pl_tap_class_of(int window) {
  return window == 1 ? 4 * PlPairOrder<P>::RE + PlPairOrder<P>::RO : 16 + P % 4;
}
template <int P>
constexpr int pl_ref_regs_of(int stage, int window) {
  return (stage == PL_SPATIAL && window == 1 && PlPairOrder<P>::shared && PL_SPATIAL_REF_REGS) ? 1 : 0;
}
inline bool pl_window_held(int P) { return P >= 3 && P <= 15 && (P & 1); }  // the instantiated windows (pl_launch)

// dynamic LDS of a launch: the shifted copies of the reference tile (both channels), the target tile, 16 spare bytes,
// and for the spatial stage the three plane tiles with their 1-pixel ring
inline size_t pl_lds_bytes(int stage, int P, int window, int rw) {
  const int TW = pl_tile_w(stage), TH = pl_tile_h(stage);
  const int TR = TH + P - 1, LW = TW + P - 1;
  const int nref = ((window == 1 ? 8 : 4) * TR * pl_ref_row_dwords(LW, window) + 1) & ~1;
  size_t words = 2 * (size_t)nref + 2 * (size_t)TR * rw + 4;
  if (stage == PL_SPATIAL) words += 3 * (size_t)(TH + 2) * (TW + 2);
  return words * 4;
}

// The launch of stage `stage` (PL_*, what the caller ASKS for) on images of rows x cols.  pp.patch must be a held window.
// tgt_aligned4: the target planes of the launch start on 4-byte boundaries.  A stage that launches nothing -- view
// propagation with one view -- gives the all-zero record.
inline PlanesVariant plan_planes(const PlanesParams& pp, bool f16, int stage, int rows, int cols, bool tgt_aligned4) {
  PlanesVariant v;
  if (!pl_window_held(pp.patch) || stage < PL_INIT || stage > PL_VIEW_REFINE || rows < 1 || cols < 1) return v;
  if (stage == PL_VIEW && pp.n_views < 2) return v;
  if (stage == PL_VIEW_REFINE && pp.n_views < 2) stage = PL_REFINE;
  v.launched = 1;
  v.stage = stage;
  v.patch = pp.patch;
  v.window = pp.window == 1 ? 1 : 0;
  v.state_f16 = f16 ? 1 : 0;
  v.tile_w = pl_tile_w(stage);
  v.tile_h = pl_tile_h(stage);
  v.grid_x = (cols + v.tile_w - 1) / v.tile_w;
  v.grid_y = (rows + v.tile_h - 1) / v.tile_h;
  v.margin = pp.margin;
  v.rw = pl_target_row_entries(v.tile_w, pp.patch, pp.max_disp, pp.margin);
  v.lds_bytes = (int)pl_lds_bytes(stage, pp.patch, v.window, v.rw);
  v.fast_fill = pl_fast_fill(cols, v.rw, tgt_aligned4) ? 1 : 0;
  switch (pp.patch) {
#define PM_PL_CASE(P) \
  case P: \
    v.ref_regs = pl_ref_regs_of<P>(stage, v.window); \
    v.tap_class = pl_tap_class_of<P>(v.window); \
    break;
    PM_PL_CASE(3) PM_PL_CASE(5) PM_PL_CASE(7) PM_PL_CASE(9) PM_PL_CASE(11) PM_PL_CASE(13) PM_PL_CASE(15)
#undef PM_PL_CASE
  }
  return v;
}

}  // namespace pm
