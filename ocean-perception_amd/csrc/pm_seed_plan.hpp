// pm_seed_plan.hpp -- what the launches of one seed map look like: ONE pure host function, plan_seed.  seed_map
// (pm_seed.hpp) launches from its result and decides nothing itself, pm_debug_seed_plan (include/pm/testing.h) returns it
// without a handle or a device, tests/test_seed_stages.py pins it.  No HIP header: this compiles with a host compiler
// alone.  No choice made here changes a result: the three selection routes compute the same corner list.
#pragma once

#include <cstddef>

namespace pm {

struct SeedParams {
  int max_features, min_distance, block_size;
  int templ_cols, templ_rows, max_disp;
  double quality_level, max_matching_cost;
  int use_harris;   // corner response det(M) - k trace(M)^2 (cv::cornerHarris) instead of the smaller eigenvalue
  double harris_k;
  // cv::cornerSubPix on the detected corners (feature_detector.cpp:110-120) / on the match (stereo_matcher.cpp:94-103)
  int subpixel_corners, subpix_winsize, subpix_zerozone, subpix_maxiters;
  float subpix_epsilon;
  int subpixel_refinement;
};

constexpr int kSeedMaxFeatures = 1024;  // capacity of the accepted-corner list

// ---- launch constants the plan shares with the kernels of pm_seed.hpp
constexpr int kEigTileW = 64, kEigTileH = 32;  // pixels one workgroup of k_seed_response owns
constexpr int kSelChunk = 2048;                // keys k_seed_select_fused sorts at a time
constexpr int kSelBins = 2048;
constexpr int kSelHist = kSelBins + kSelBins / 32;  // bin b lives at b + (b >> 5): 32-bin runs fall on distinct banks
constexpr size_t kSeedSelectLdsLimit = 150 * 1024;  // what a selection workgroup may take of the CU's 160 KB
constexpr int kSeedPackedMax = 32768;  // x | y << 16 packing, and squared distances (any two candidates of a batch) that fit an int

// dynamic LDS of k_seed_select_fused: two chunks of keys, the histogram, 8 words, the padded grid of accepted corners
inline size_t seed_select_lds_bytes(int gx, int gy) {
  return sizeof(unsigned long long) * 2 * kSelChunk + sizeof(unsigned) * (kSelHist + 8) +
         sizeof(int) * 4 * (size_t)(gx + 2) * (size_t)(gy + 2);
}
// dynamic LDS of k_seed_select_grid: the grid alone
inline size_t seed_grid_lds_bytes(int gx, int gy) { return (size_t)gx * (size_t)gy * 4 * sizeof(int); }

// The selection of the accepted corners among the candidates, three routes with one result:
enum SeedRoute {
  kSeedRouteAuto = 0,        // (an argument of plan_seed only, never in a plan)
  kSeedRouteFused = 1,       // k_seed_select_fused: sort + selection in one workgroup, chunk by chunk
  kSeedRouteSortedGrid = 2,  // radix sort of all slots, then k_seed_select_grid (accepted corners in a grid in LDS)
  kSeedRouteSortedList = 3,  // radix sort of all slots, then k_seed_select (accepted corners in a list: any min distance)
};

struct SeedPlan {
  const char* refused = nullptr;  // non-null: the forced route cannot run with these parameters (nothing else is set)
  int route = 0;
  int gx = 0, gy = 0;             // cells of min_distance pixels over the image; 0 x 0 where min_distance < 1
  size_t select_lds = 0;          // dynamic LDS of the selection launch
  int max_features = 0;           // corners the selection stops at: max_features, at most kSeedMaxFeatures
  int response_window = 0;        // the compiled-in box window of k_seed_response (3, 5, 7), 0 = the generic loop
  int tiles_x = 0, tiles_y = 0;   // its grid
  size_t response_lds = 0;        // its dynamic LDS: the derivative tile plus a halo of block_size / 2
  size_t match_lds = 0;           // dynamic LDS of k_seed_match: template and search stripe, rows padded to dwords
};

// forced_route: kSeedRouteAuto = the route a map takes (fused_enabled: the tuning build's PM_SEED_FUSED switch), else that
// route or a refusal -- never a fallback.
inline SeedPlan plan_seed(const SeedParams& sp, int rows, int cols, int forced_route, bool fused_enabled = true) {
  SeedPlan pl;
  const int md = sp.min_distance;
  const int gx = md >= 1 ? (cols + md - 1) / md : 0, gy = md >= 1 ? (rows + md - 1) / md : 0;
  const bool packed_ok = md >= 1 && cols <= kSeedPackedMax && rows <= kSeedPackedMax;
  const bool fused_ok = packed_ok && seed_select_lds_bytes(gx, gy) <= kSeedSelectLdsLimit;
  const bool grid_ok = packed_ok && seed_grid_lds_bytes(gx, gy) <= kSeedSelectLdsLimit;
  int route;
  switch (forced_route) {
    case kSeedRouteAuto:
      route = fused_ok && fused_enabled ? kSeedRouteFused : grid_ok ? kSeedRouteSortedGrid : kSeedRouteSortedList;
      break;
    case kSeedRouteFused:
    case kSeedRouteSortedGrid:
      if (md < 1) pl.refused = "the grid selections need a min distance of at least 1";
      else if (!packed_ok) pl.refused = "the grid selections take images of at most 32768 rows and columns";
      else if (!(forced_route == kSeedRouteFused ? fused_ok : grid_ok)) pl.refused = "the grid of this min distance does not fit the LDS";
      route = forced_route;
      break;
    case kSeedRouteSortedList:
      route = forced_route;
      break;
    default:
      pl.refused = "no such selection route";
      route = 0;
  }
  if (pl.refused) return pl;
  pl.route = route;
  pl.gx = gx;
  pl.gy = gy;
  pl.select_lds = route == kSeedRouteFused ? seed_select_lds_bytes(gx, gy)
                  : route == kSeedRouteSortedGrid ? seed_grid_lds_bytes(gx, gy) : 0;
  pl.max_features = sp.max_features < kSeedMaxFeatures ? sp.max_features : kSeedMaxFeatures;
  const int bs = sp.block_size;
  pl.response_window = bs == 3 || bs == 5 || bs == 7 ? bs : 0;
  pl.tiles_x = (cols + kEigTileW - 1) / kEigTileW;
  pl.tiles_y = (rows + kEigTileH - 1) / kEigTileH;
  const int hb = bs / 2;
  pl.response_lds = sizeof(unsigned) * (size_t)(kEigTileW + 2 * hb) * (size_t)(kEigTileH + 2 * hb);
  pl.match_lds = 4 * ((size_t)sp.templ_rows * (size_t)((sp.templ_cols + 3) / 4) +
                      (size_t)(sp.templ_rows + 2) * (size_t)((sp.max_disp + 3) / 4 + 1));
  return pl;
}

}  // namespace pm
