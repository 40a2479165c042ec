// consistency_host_main.cpp -- runs pm_filter_consistency's own per-thread code (csrc/pm_consistency_body.hpp:
// consistency_lane<RADIUS>, the body of k_consistency of csrc/pm_consistency.hpp) on the HOST, so that
// tests/test_consistency.py can hold it to the definition (tests/consistency_ref.py) without a GPU and under
// -fsanitize=address,undefined.  Every buffer is a heap allocation of EXACTLY the bytes the stage may touch.  The launch --
// its grid and block are the body header's span_blocks() and kConsistencyBlockX / Y, walked by host_launch.hpp -- runs
// twice, blocks and threads forwards and then backwards: the result must not depend on the order (only integer addition
// crosses threads).  Then once more in place (d_out == d_disp) and once with the counts alone.  Compiled as HIP source with
// the host-only switch of hipcc and -ffp-contract=off.
//   consistency_host_main <dir>
// <dir> holds .npy dumps (host_npy.hpp: Case): params.npy (float64: rows, cols, fx, fy, cx, cy, baseline, n, radius, max_diff,
// min_consistent, max_conflicts, then 8 x (R[9], t[3]), the unused ones 0), disp.npy (float32 [rows][cols]), sources.npy
// (float32 [n][rows][cols]) and the definition's results want_out.npy, want_residual.npy (float32 [rows][cols]),
// want_classes.npy (uint16 [rows][cols]) and want_counts.npy (int32 [2]).
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.

#include "host_launch.hpp"
#include "host_npy.hpp"
#include "pm_consistency_body.hpp"

enum { kRows, kCols, kFx, kFy, kCx, kCy, kBaseline, kN, kRadius, kMaxDiff, kMinConsistent, kMaxConflicts, kMotions };
static const int kParams = kMotions + 12 * pm::kConsistencyMaxSources;

static unsigned lane(const pm::ConsistencyArgs& a, int radius, int x, int y) {
  switch (radius) {
    case 0: return pm::consistency_lane<0>(a, x, y);
    case 1: return pm::consistency_lane<1>(a, x, y);
    default: return pm::consistency_lane<2>(a, x, y);
  }
}

// every thread of every block of k_consistency
static void run(const pm::ConsistencyArgs& a, int radius, bool backwards) {
  const pm::SpanBlocks grid = pm::span_blocks(a.rows, a.cols);
  for_blocks(grid.x, grid.y, 1, backwards, [&](int bx, int by, int) {
    int sums[2] = {0, 0};  // valid, kept
    for_threads(pm::kConsistencyBlockX, pm::kConsistencyBlockY, backwards, [&](int tx, int ty) {
      const int x = bx * pm::kConsistencySpan + tx, y = by * pm::kConsistencyBlockY + ty;
      add_flags<pm::kConsistencyPixelsPerLane>(x < a.cols && y < a.rows ? lane(a, radius, x, y) : 0u, sums);
    });
    flush_sums(a.counts, sums, pm::reproject_add);
  });
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Case c(argv[1]);
  const std::vector<double> p = c.params(kParams);
  const int rows = (int)p[kRows], cols = (int)p[kCols], n = (int)p[kN], radius = (int)p[kRadius];
  const pm_cloud_camera camera = {p[kFx], p[kFy], p[kCx], p[kCy], p[kBaseline]};
  if (c.failed || rows < 1 || cols < 1 || n < 1 || n > pm::kConsistencyMaxSources || radius < 0 || radius > pm::kConsistencyMaxRadius)
    return 2;
  const size_t px = (size_t)rows * cols;
  const auto disp = c.read<float>("disp", px);
  const auto src_b = c.raw("sources", 4 * px * n);
  const auto want_out = c.raw("want_out", 4 * px), want_cls = c.raw("want_classes", 2 * px);
  const auto want_res = c.raw("want_residual", 4 * px), want_counts = c.raw("want_counts", 8);
  if (c.failed) return 2;
  std::unique_ptr<float[]> maps[pm::kConsistencyMaxSources];  // one exactly sized allocation per source
  pm::ConsistencyArgs a = {};
  a.cam = pm::cloud_cam(camera);
  a.rows = rows, a.cols = cols, a.n = n;
  a.max_diff = (float)p[kMaxDiff], a.min_consistent = (int)p[kMinConsistent], a.max_conflicts = (int)p[kMaxConflicts];
  for (int k = 0; k < n; ++k) {
    maps[k] = exact_copy<float>(src_b.get() + 4 * px * k, px);
    a.src[k].map = maps[k].get();
    read_motion(&p[kMotions + 12 * k], a.src[k].R, a.src[k].t);
  }
  int bad = 0;
  for (int pass = 0; pass < 4; ++pass) {  // forwards, backwards, in place, the counts alone
    const bool backwards = pass == 1;
    const char* const name = pass == 0 ? "forwards" : pass == 1 ? "backwards" : pass == 2 ? "in place" : "counts alone";
    const auto cur = exact_copy<float>(disp.get(), px);
    std::unique_ptr<float[]> out(new float[px]), res(new float[px]);
    std::unique_ptr<uint16_t[]> cls(new uint16_t[px]);
    int counts[2] = {0, 0};
    a.disp = cur.get();
    a.out = pass == 2 ? cur.get() : pass == 3 ? nullptr : out.get();
    a.classes = pass == 3 ? nullptr : cls.get();
    a.residual = pass == 3 ? nullptr : res.get();
    a.counts = counts;
    run(a, radius, backwards);
    if (pass != 3) {
      bad |= differ("out", a.out, want_out.get(), 4 * px, name);
      bad |= differ("classes", cls.get(), want_cls.get(), 2 * px, name);
      bad |= differ("residual", res.get(), want_res.get(), 4 * px, name);
    }
    if (pass != 2) bad |= differ("the input map", cur.get(), disp.get(), 4 * px, name);  // read only
    bad |= differ("counts", counts, want_counts.get(), 8, name);
  }
  return bad ? 1 : 0;
}
