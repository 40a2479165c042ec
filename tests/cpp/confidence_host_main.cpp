// confidence_host_main.cpp -- runs pm_disparity_confidence's own per-thread code (csrc/pm_confidence_body.hpp: the steps
// k_confidence of csrc/pm_confidence.hpp takes between its barriers, and sobel_mag of csrc/pm_device.hpp for the gradient
// launch) on the HOST, so that tests/test_confidence.py can hold it to the definition (tests/confidence_ref.py) without a GPU
// and under -fsanitize=address,undefined.  Every buffer is a heap allocation of EXACTLY the bytes the stage may touch; a
// block's LDS tile is one of exactly the bytes its window needs.  The launch (host_launch.hpp's walk over the body header's
// kConfTileW x kConfTileH) runs forwards, backwards (blocks and threads: the result must not depend on the order, only
// integer addition crosses threads), in place (d_out == d_disp_l), with every block sent down the global-memory path, and
// with the counts alone.  Compiled as HIP source with the host-only switch of hipcc and -ffp-contract=off.
//   confidence_host_main <dir>
// <dir> holds .npy dumps (host_npy.hpp: Case): params.npy (float64: rows, cols, pw, ph, max_cost, min_margin, min_bg_margin,
// max_lr_diff, drop_unmeasured, with_right, alpha, tau_color, tau_grad), left.npy, right.npy (uint8 [rows][cols]), disp_l.npy,
// disp_r.npy (float32 [rows][cols]; disp_r is read only with with_right) and the definition's results want_out.npy (float32
// [rows][cols]), want_measures.npy (float32 [4][rows][cols]), want_flags.npy (uint8 [rows][cols]) and want_counts.npy (int32
// [3]).
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.

#include "host_launch.hpp"
#include "host_npy.hpp"
#include "pm_confidence_body.hpp"

enum { kRows, kCols, kPw, kPh, kMaxCost, kMinMargin, kMinBgMargin, kMaxLrDiff, kDropUnmeasured, kWithRight, kAlpha, kTauColor,
       kTauGrad, kParams };

template <typename Src>
static unsigned finish(const pm::ConfidenceArgs& a, const pm::ConfidenceLane& l, const Src& s, int x, int y) {
  switch (a.pw == a.ph ? a.pw : 0) {  // pm_disparity_confidence's own choice of a kernel
    case 3: return pm::confidence_lane_finish<3, 3>(a, l, s, x, y);
    case 5: return pm::confidence_lane_finish<5, 5>(a, l, s, x, y);
    case 7: return pm::confidence_lane_finish<7, 7>(a, l, s, x, y);
    case 9: return pm::confidence_lane_finish<9, 9>(a, l, s, x, y);
    case 11: return pm::confidence_lane_finish<11, 11>(a, l, s, x, y);
    default: return pm::confidence_lane_finish<0, 0>(a, l, s, x, y);
  }
}

// every thread of every block of k_confidence: grid (ceil(cols / 32), ceil(rows / 8)), block 32 x 8; returns the tiled blocks
static int run(const pm::ConfidenceArgs& a, bool backwards, bool all_global) {
  const int gx = (a.cols + pm::kConfTileW - 1) / pm::kConfTileW, gy = (a.rows + pm::kConfTileH - 1) / pm::kConfTileH;
  const int tr = pm::confidence_tile_rows(a.ph), lwp = pm::confidence_tile_lwp(a.pw);
  int tiled_blocks = 0;
  for_blocks(gx, gy, 1, backwards, [&](int bx, int by, int) {
    const int x0 = bx * pm::kConfTileW, y0 = by * pm::kConfTileH;
    std::vector<pm::ConfidenceLane> lanes(pm::kConfThreads);
    int lo = 0x7fffffff, hi = -0x7fffffff;
    for_threads(pm::kConfTileW, pm::kConfTileH, backwards, [&](int tx, int ty) {  // up to the first barrier
      pm::ConfidenceLane& l = lanes[ty * pm::kConfTileW + tx];
      l = pm::confidence_lane_setup(a, x0 + tx, y0 + ty);
      if (l.measured) {
        lo = l.lo < lo ? l.lo : lo;
        hi = l.hi > hi ? l.hi : hi;
      }
    });
    // the block's LDS: exactly the bytes of this window's tile
    std::unique_ptr<uint8_t[]> l8(new uint8_t[tr * lwp]), lg(new uint8_t[tr * lwp]), r8(new uint8_t[tr * pm::kConfTileRW]),
        rg8(new uint8_t[tr * pm::kConfTileRW]);
    std::unique_ptr<float[]> rg(new float[tr * pm::kConfTileRW]);
    pm::ConfidenceTile tile = {l8.get(), lg.get(), r8.get(), rg8.get(), rg.get(), lwp, 0, 0};
    const bool tiled = hi >= lo && pm::confidence_tile_plan(lo, hi, a.pw, &tile.lo4, &tile.rw) && !all_global;
    tiled_blocks += tiled ? 1 : 0;
    if (tiled)
      for_threads(pm::kConfTileW, pm::kConfTileH, backwards,
                  [&](int tx, int ty) { pm::confidence_fill(a, tile, x0, y0, ty * pm::kConfTileW + tx); });
    int sums[3] = {0, 0, 0};
    for_threads(pm::kConfTileW, pm::kConfTileH, backwards, [&](int tx, int ty) {  // behind the second barrier
      const int x = x0 + tx, y = y0 + ty;
      const pm::ConfidenceLane& l = lanes[ty * pm::kConfTileW + tx];
      add_flags<1>(tiled ? finish(a, l, pm::ConfidenceTileSrc{tile, tx, ty}, x, y) : finish(a, l, pm::ConfidenceGlobalSrc{a, x, y}, x, y),
                   sums);
    });
    flush_sums(a.counts, sums, pm::reproject_add);
  });
  return tiled_blocks;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Case c(argv[1]);
  const std::vector<double> p = c.params(kParams);
  const int rows = (int)p[kRows], cols = (int)p[kCols], pw = (int)p[kPw], ph = (int)p[kPh];
  const bool with_right = p[kWithRight] != 0.0;
  if (c.failed || rows < 1 || cols < 1 || pw < 3 || pw > PM_MAX_PATCH || !(pw & 1) || ph < 3 || ph > PM_MAX_PATCH || !(ph & 1)) return 2;
  const size_t px = (size_t)rows * cols;
  const auto left = c.read<uint8_t>("left", px), right = c.read<uint8_t>("right", px);
  const auto disp_l = c.read<float>("disp_l", px), disp_r = c.read<float>("disp_r", px);
  const auto want_out = c.raw("want_out", 4 * px), want_meas = c.raw("want_measures", 16 * px);
  const auto want_flags = c.raw("want_flags", px), want_counts = c.raw("want_counts", 12);
  if (c.failed) return 2;
  std::unique_ptr<float[]> gr(new float[px]);
  std::unique_ptr<uint8_t[]> gl8(new uint8_t[px]);
  for (int y = 0; y < rows; ++y)  // k_confidence_grad, every thread inside the image
    for (int x = 0; x < cols; ++x) {
      gl8[(size_t)y * cols + x] = (uint8_t)pm::sat_u8(pm::sobel_mag(left.get(), (size_t)cols, rows, cols, x, y));
      gr[(size_t)y * cols + x] = pm::sobel_mag(right.get(), (size_t)cols, rows, cols, x, y);
    }
  pm::ConfidenceArgs a = {};
  a.left = left.get(), a.right = right.get(), a.gl8 = gl8.get(), a.gr = gr.get();
  a.disp_r = with_right ? disp_r.get() : nullptr;
  a.rows = rows, a.cols = cols, a.pw = pw, a.ph = ph;
  a.max_cost = (float)p[kMaxCost], a.min_margin = (float)p[kMinMargin], a.min_bg_margin = (float)p[kMinBgMargin];
  a.max_lr_diff = (float)p[kMaxLrDiff], a.drop_unmeasured = (int)p[kDropUnmeasured];
  a.cp = pm::confidence_cost_params((float)p[kAlpha], (float)p[kTauColor], (float)p[kTauGrad], pw, ph);
  int bad = 0;
  for (int pass = 0; pass < 5; ++pass) {  // forwards, backwards, in place, all blocks global, the counts alone
    static const char* const names[5] = {"forwards", "backwards", "in place", "global path", "counts alone"};
    const auto cur = exact_copy<float>(disp_l.get(), px);
    std::unique_ptr<float[]> out(new float[px]), meas(new float[4 * px]);
    std::unique_ptr<uint8_t[]> flags(new uint8_t[px]);
    int counts[3] = {0, 0, 0};
    a.disp_l = cur.get();
    a.out = pass == 2 ? cur.get() : pass == 4 ? nullptr : out.get();
    a.measures = pass == 4 ? nullptr : meas.get();
    a.flags = pass == 4 ? nullptr : flags.get();
    a.counts = counts;
    const int tiled = run(a, pass == 1, pass == 3);
    if (pass == 0) printf("tiled blocks: %d\n", tiled);
    if (pass != 4) {
      bad |= differ("out", a.out, want_out.get(), 4 * px, names[pass]);
      bad |= differ("measures", meas.get(), want_meas.get(), 16 * px, names[pass]);
      bad |= differ("flags", flags.get(), want_flags.get(), px, names[pass]);
    }
    if (pass != 2) bad |= differ("the input map", cur.get(), disp_l.get(), 4 * px, names[pass]);  // read only
    bad |= differ("counts", counts, want_counts.get(), 12, names[pass]);
  }
  return bad ? 1 : 0;
}
