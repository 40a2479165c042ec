// consistency_host_main.cpp -- runs pm_filter_consistency's own per-thread code (csrc/pm_consistency_body.hpp:
// consistency_lane<RADIUS>, the body of k_consistency of csrc/pm_consistency.hpp) on the HOST, so that
// tests/test_consistency.py can hold it to the definition (tests/consistency_ref.py) without a GPU and under
// -fsanitize=address,undefined.  Every buffer is a heap allocation of EXACTLY the bytes the stage may touch.  The launch runs
// twice, blocks and threads forwards and then backwards: the result must not depend on the order (only integer addition
// crosses threads).  Then once more in place (d_out == d_disp) and once with the counts alone.  Compiled as HIP source with
// the host-only switch of hipcc and -ffp-contract=off.
//   consistency_host_main <dir>
// <dir> holds .npy dumps (numpy's format, version 1, C order, little endian; the header is skipped and the payload size
// checked): params.npy (float64: rows, cols, fx, fy, cx, cy, baseline, n, radius, max_diff, min_consistent, max_conflicts,
// then 8 x (R[9], t[3]), the unused ones 0), disp.npy (float32 [rows][cols]), sources.npy (float32 [n][rows][cols]) and the
// definition's results want_out.npy, want_residual.npy (float32 [rows][cols]), want_classes.npy (uint16 [rows][cols]) and
// want_counts.npy (int32 [2]).
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "host_npy.hpp"
#include "pm_consistency_body.hpp"

static const int kParams = 12 + 12 * pm::kConsistencyMaxSources;

static int nth(int i, int n, bool backwards) { return backwards ? n - 1 - i : i; }

static unsigned lane(const pm::ConsistencyArgs& a, int radius, int x, int y) {
  switch (radius) {
    case 0: return pm::consistency_lane<0>(a, x, y);
    case 1: return pm::consistency_lane<1>(a, x, y);
    default: return pm::consistency_lane<2>(a, x, y);
  }
}

// every thread of every block of k_consistency: grid (ceil(cols / 256), ceil(rows / 4)), block (64, 4)
static void run(const pm::ConsistencyArgs& a, int radius, bool backwards) {
  const int bx = pm::kConsistencyLanes, by = 4, span = bx * pm::kConsistencyPixelsPerLane;
  const int gx = (a.cols + span - 1) / span, gy = (a.rows + by - 1) / by;
  for (int b = 0; b < gx * gy; ++b) {
    const int block = nth(b, gx * gy, backwards);
    int valid = 0, kept = 0;
    for (int i = 0; i < bx * by; ++i) {
      const int t = nth(i, bx * by, backwards);
      const int x = (block % gx) * span + t % bx, y = (block / gx) * by + t / bx;
      const unsigned flags = x < a.cols && y < a.rows ? lane(a, radius, x, y) : 0u;
      valid += __builtin_popcount(flags & 15u);
      kept += __builtin_popcount(flags >> 4);
    }
    if (valid) pm::reproject_add(a.counts, valid);
    if (kept) pm::reproject_add(a.counts + 1, kept);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = std::string(argv[1]) + "/";
  std::unique_ptr<uint8_t[]> raw;
  if (!read_npy(dir + "params.npy", kParams * sizeof(double), &raw)) return 2;
  double p[kParams];
  memcpy(p, raw.get(), sizeof p);
  const int rows = (int)p[0], cols = (int)p[1], n = (int)p[7], radius = (int)p[8];
  const pm_cloud_camera camera = {p[2], p[3], p[4], p[5], p[6]};
  if (rows < 1 || cols < 1 || n < 1 || n > pm::kConsistencyMaxSources || radius < 0 || radius > pm::kConsistencyMaxRadius) return 2;
  const size_t px = (size_t)rows * cols;
  std::unique_ptr<uint8_t[]> disp_b, src_b, want_out, want_cls, want_res, want_counts;
  if (!read_npy(dir + "disp.npy", 4 * px, &disp_b) || !read_npy(dir + "sources.npy", 4 * px * n, &src_b) ||
      !read_npy(dir + "want_out.npy", 4 * px, &want_out) || !read_npy(dir + "want_classes.npy", 2 * px, &want_cls) ||
      !read_npy(dir + "want_residual.npy", 4 * px, &want_res) || !read_npy(dir + "want_counts.npy", 8, &want_counts))
    return 2;
  std::unique_ptr<float[]> disp(new float[px]);
  memcpy(disp.get(), disp_b.get(), 4 * px);
  std::unique_ptr<float[]> maps[pm::kConsistencyMaxSources];  // one exactly sized allocation per source
  pm::ConsistencyArgs a = {};
  a.cam = pm::cloud_cam(camera);
  a.rows = rows, a.cols = cols, a.n = n;
  a.max_diff = (float)p[9], a.min_consistent = (int)p[10], a.max_conflicts = (int)p[11];
  for (int k = 0; k < n; ++k) {
    maps[k].reset(new float[px]);
    memcpy(maps[k].get(), src_b.get() + 4 * px * k, 4 * px);
    a.src[k].map = maps[k].get();
    for (int i = 0; i < 9; ++i) a.src[k].R[i] = p[12 + 12 * k + i];
    for (int i = 0; i < 3; ++i) a.src[k].t[i] = p[12 + 12 * k + 9 + i];
  }
  int bad = 0;
  for (int pass = 0; pass < 4; ++pass) {  // forwards, backwards, in place, the counts alone
    const bool backwards = pass == 1;
    const char* const name = pass == 0 ? "forwards" : pass == 1 ? "backwards" : pass == 2 ? "in place" : "counts alone";
    std::unique_ptr<float[]> cur(new float[px]), out(new float[px]), res(new float[px]);
    std::unique_ptr<uint16_t[]> cls(new uint16_t[px]);
    memcpy(cur.get(), disp.get(), 4 * px);
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
