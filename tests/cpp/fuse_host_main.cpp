// fuse_host_main.cpp -- runs pm_fuse_disparity's own per-thread code (csrc/pm_fuse_body.hpp: fuse_splat_lane and
// fuse_lane<RADIUS>, the bodies of k_fuse_splat and k_fuse of csrc/pm_fuse.hpp) on the HOST, so that tests/test_fuse.py can
// hold it to the definition (tests/fuse_ref.py) without a GPU and under -fsanitize=address,undefined.  Every buffer is a heap
// allocation of EXACTLY the bytes the stage may touch.  Both launches -- their grid and block are the body header's
// span_blocks() and kFuseBlockX / Y, walked by host_launch.hpp -- run twice, blocks and threads forwards and then backwards:
// the result must not depend on the order (only integer maximum and integer addition cross threads).  Then once more in place
// (d_out == d_disp) and once with the counts alone.  Compiled as HIP source with the host-only switch of hipcc and
// -ffp-contract=off.
//   fuse_host_main <dir>
// <dir> holds .npy dumps (host_npy.hpp: Case): params.npy (float64: rows, cols, fx, fy, cx, cy, baseline, n, radius, max_diff,
// min_consistent, max_conflicts, fill_min_sources, fill_max_diff, has_weight, then 8 x has_weight_k, then 8 x (R[9], t[3]),
// the unused ones 0), disp.npy (float32 [rows][cols]), sources.npy (float32 [n][rows][cols]), weights.npy (float32
// [1 + n][rows][cols]: the current map's plane, then the sources'; a plane that is not given is there and not read) and the
// definition's results want_out.npy, want_spread.npy (float32 [rows][cols]), want_count.npy, want_flags.npy (uint8
// [rows][cols]) and want_counts.npy (int32 [4]).
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.

#include "host_launch.hpp"
#include "host_npy.hpp"
#include "pm_fuse_body.hpp"

enum { kRows, kCols, kFx, kFy, kCx, kCy, kBaseline, kN, kRadius, kMaxDiff, kMinConsistent, kMaxConflicts, kFillMinSources,
       kFillMaxDiff, kHasWeight, kSourceHasWeight, kMotions = kSourceHasWeight + pm::kFuseMaxSources };
static const int kParams = kMotions + 12 * pm::kFuseMaxSources;

static unsigned lane(const pm::FuseArgs& a, int radius, int x, int y) {
  switch (radius) {
    case 0: return pm::fuse_lane<0>(a, x, y);
    case 1: return pm::fuse_lane<1>(a, x, y);
    default: return pm::fuse_lane<2>(a, x, y);
  }
}

// every thread of every block of k_fuse_splat: the source is the block's z
static void run_splat(const pm::FuseSplatArgs& a, int n, bool backwards) {
  const pm::SpanBlocks grid = pm::span_blocks(a.rows, a.cols);
  for_blocks(grid.x, grid.y, n, backwards, [&](int bx, int by, int bz) {
    for_threads(pm::kFuseBlockX, pm::kFuseBlockY, backwards, [&](int tx, int ty) {
      const int x = bx * pm::kFuseSpan + tx, y = by * pm::kFuseBlockY + ty;
      if (x < a.cols && y < a.rows) pm::fuse_splat_lane(a, bz, x, y);
    });
  });
}

// every thread of every block of k_fuse
static void run(const pm::FuseArgs& a, int radius, bool backwards) {
  const pm::SpanBlocks grid = pm::span_blocks(a.rows, a.cols);
  for_blocks(grid.x, grid.y, 1, backwards, [&](int bx, int by, int) {
    int sums[pm::kFuseCounters] = {};
    for_threads(pm::kFuseBlockX, pm::kFuseBlockY, backwards, [&](int tx, int ty) {
      const int x = bx * pm::kFuseSpan + tx, y = by * pm::kFuseBlockY + ty;
      add_flags<pm::kFusePixelsPerLane>(x < a.cols && y < a.rows ? lane(a, radius, x, y) : 0u, sums);
    });
    flush_sums(a.counts, sums, pm::reproject_add);
  });
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Case c(argv[1]);
  const std::vector<double> p = c.params(kParams);
  const int rows = (int)p[kRows], cols = (int)p[kCols], n = (int)p[kN], radius = (int)p[kRadius], fill_min = (int)p[kFillMinSources];
  const pm_cloud_camera camera = {p[kFx], p[kFy], p[kCx], p[kCy], p[kBaseline]};
  if (c.failed || rows < 1 || cols < 1 || n < 1 || n > pm::kFuseMaxSources || radius < 0 || radius > pm::kFuseMaxRadius ||
      fill_min < 0 || fill_min > n)
    return 2;
  const size_t px = (size_t)rows * cols;
  const auto disp = c.read<float>("disp", px);
  const auto src_b = c.raw("sources", 4 * px * n), w_b = c.raw("weights", 4 * px * (n + 1));
  const auto want_out = c.raw("want_out", 4 * px), want_count = c.raw("want_count", px);
  const auto want_spread = c.raw("want_spread", 4 * px), want_flags = c.raw("want_flags", px), want_counts = c.raw("want_counts", 16);
  if (c.failed) return 2;
  std::unique_ptr<float[]> maps[pm::kFuseMaxSources], weights[pm::kFuseMaxSources + 1];  // exactly sized allocations
  pm::FuseArgs a = {};
  a.cam = pm::cloud_cam(camera);
  a.rows = rows, a.cols = cols, a.n = n, a.px = px;
  a.max_diff = (float)p[kMaxDiff], a.min_consistent = (int)p[kMinConsistent], a.max_conflicts = (int)p[kMaxConflicts];
  a.fill_min_sources = fill_min, a.fill_max_diff = (float)p[kFillMaxDiff];
  if (p[kHasWeight] != 0.0) {
    weights[0] = exact_copy<float>(w_b.get(), px);
    a.weight = weights[0].get();
  }
  pm::FuseSplatArgs sa = {};
  sa.cam = a.cam, sa.rows = rows, sa.cols = cols, sa.px = px;
  for (int k = 0; k < n; ++k) {
    maps[k] = exact_copy<float>(src_b.get() + 4 * px * k, px);
    read_motion(&p[kMotions + 12 * k], a.src[k].R, a.src[k].t);
    a.src[k].map = maps[k].get();
    if (p[kSourceHasWeight + k] != 0.0) {
      weights[k + 1] = exact_copy<float>(w_b.get() + 4 * px * (k + 1), px);
      a.src[k].weight = weights[k + 1].get();
    }
    pm::motion_inverse(a.src[k].R, a.src[k].t, sa.src[k].R, sa.src[k].t);  // as pm_fuse_disparity forms it on the host
    sa.src[k].map = maps[k].get();
  }
  int bad = 0;
  for (int pass = 0; pass < 4; ++pass) {  // forwards, backwards, in place, the counts alone
    const bool backwards = pass == 1;
    const char* const name = pass == 0 ? "forwards" : pass == 1 ? "backwards" : pass == 2 ? "in place" : "counts alone";
    std::unique_ptr<float[]> out(new float[px]), spread(new float[px]);
    std::unique_ptr<uint8_t[]> count(new uint8_t[px]), flags(new uint8_t[px]);
    std::unique_ptr<unsigned[]> splat;  // no map scratch without a fill
    if (fill_min >= 1) {
      splat.reset(new unsigned[px * n]());
      sa.splat = splat.get();
      run_splat(sa, n, backwards);
    }
    const auto cur = exact_copy<float>(disp.get(), px);
    int counts[pm::kFuseCounters] = {};
    a.disp = cur.get();
    a.splat = splat.get();
    a.out = pass == 2 ? cur.get() : pass == 3 ? nullptr : out.get();
    a.count = pass == 3 ? nullptr : count.get();
    a.spread = pass == 3 ? nullptr : spread.get();
    a.flags = pass == 3 ? nullptr : flags.get();
    a.counts = counts;
    run(a, radius, backwards);
    if (pass != 3) {
      bad |= differ("out", a.out, want_out.get(), 4 * px, name);
      bad |= differ("count", count.get(), want_count.get(), px, name);
      bad |= differ("spread", spread.get(), want_spread.get(), 4 * px, name);
      bad |= differ("flags", flags.get(), want_flags.get(), px, name);
    }
    if (pass != 2) bad |= differ("the input map", cur.get(), disp.get(), 4 * px, name);  // read only
    bad |= differ("counts", counts, want_counts.get(), 16, name);
  }
  return bad ? 1 : 0;
}
