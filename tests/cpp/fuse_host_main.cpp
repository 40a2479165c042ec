// fuse_host_main.cpp -- runs pm_fuse_disparity's own per-thread code (csrc/pm_fuse_body.hpp: fuse_splat_lane and
// fuse_lane<RADIUS>, the bodies of k_fuse_splat and k_fuse of csrc/pm_fuse.hpp) on the HOST, so that tests/test_fuse.py can
// hold it to the definition (tests/fuse_ref.py) without a GPU and under -fsanitize=address,undefined.  Every buffer is a heap
// allocation of EXACTLY the bytes the stage may touch.  Both launches run twice, blocks and threads forwards and then backwards:
// the result must not depend on the order (only integer maximum and integer addition cross threads).  Then once more in place
// (d_out == d_disp) and once with the counts alone.  Compiled as HIP source with the host-only switch of hipcc and
// -ffp-contract=off.
//   fuse_host_main <dir>
// <dir> holds .npy dumps (numpy's format, version 1, C order, little endian; the header is skipped and the payload size
// checked): params.npy (float64: rows, cols, fx, fy, cx, cy, baseline, n, radius, max_diff, min_consistent, max_conflicts,
// fill_min_sources, fill_max_diff, has_weight, then 8 x has_weight_k, then 8 x (R[9], t[3]), the unused ones 0), disp.npy
// (float32 [rows][cols]), sources.npy (float32 [n][rows][cols]), weights.npy (float32 [1 + n][rows][cols]: the current map's
// plane, then the sources'; a plane that is not given is there and not read) and the definition's results want_out.npy,
// want_spread.npy (float32 [rows][cols]), want_count.npy, want_flags.npy (uint8 [rows][cols]) and want_counts.npy (int32 [4]).
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "host_npy.hpp"
#include "pm_fuse_body.hpp"

static const int kHead = 15;
static const int kParams = kHead + pm::kFuseMaxSources + 12 * pm::kFuseMaxSources;

static int nth(int i, int n, bool backwards) { return backwards ? n - 1 - i : i; }

static unsigned lane(const pm::FuseArgs& a, int radius, int x, int y) {
  switch (radius) {
    case 0: return pm::fuse_lane<0>(a, x, y);
    case 1: return pm::fuse_lane<1>(a, x, y);
    default: return pm::fuse_lane<2>(a, x, y);
  }
}

// every thread of every block of k_fuse_splat: grid (ceil(cols / 256), ceil(rows / 4), n), block (64, 4)
static void run_splat(const pm::FuseSplatArgs& a, int n, bool backwards) {
  const int bx = pm::kFuseLanes, by = 4, span = bx * pm::kFusePixelsPerLane;
  const int gx = (a.cols + span - 1) / span, gy = (a.rows + by - 1) / by;
  for (int b = 0; b < gx * gy * n; ++b) {
    const int block = nth(b, gx * gy * n, backwards);
    for (int i = 0; i < bx * by; ++i) {
      const int t = nth(i, bx * by, backwards);
      const int x = (block % gx) * span + t % bx, y = (block / gx % gy) * by + t / bx;
      if (x < a.cols && y < a.rows) pm::fuse_splat_lane(a, block / (gx * gy), x, y);
    }
  }
}

// every thread of every block of k_fuse: grid (ceil(cols / 256), ceil(rows / 4)), block (64, 4)
static void run(const pm::FuseArgs& a, int radius, bool backwards) {
  const int bx = pm::kFuseLanes, by = 4, span = bx * pm::kFusePixelsPerLane;
  const int gx = (a.cols + span - 1) / span, gy = (a.rows + by - 1) / by;
  for (int b = 0; b < gx * gy; ++b) {
    const int block = nth(b, gx * gy, backwards);
    int sums[4] = {0, 0, 0, 0};
    for (int i = 0; i < bx * by; ++i) {
      const int t = nth(i, bx * by, backwards);
      const int x = (block % gx) * span + t % bx, y = (block / gx) * by + t / bx;
      const unsigned flags = x < a.cols && y < a.rows ? lane(a, radius, x, y) : 0u;
      for (int c = 0; c < 4; ++c) sums[c] += __builtin_popcount((flags >> (4 * c)) & 15u);
    }
    for (int c = 0; c < 4; ++c)
      if (sums[c]) pm::reproject_add(a.counts + c, sums[c]);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = std::string(argv[1]) + "/";
  std::unique_ptr<uint8_t[]> raw;
  if (!read_npy(dir + "params.npy", kParams * sizeof(double), &raw)) return 2;
  double p[kParams];
  memcpy(p, raw.get(), sizeof p);
  const int rows = (int)p[0], cols = (int)p[1], n = (int)p[7], radius = (int)p[8], fill_min = (int)p[12];
  const pm_cloud_camera camera = {p[2], p[3], p[4], p[5], p[6]};
  if (rows < 1 || cols < 1 || n < 1 || n > pm::kFuseMaxSources || radius < 0 || radius > pm::kFuseMaxRadius || fill_min < 0 ||
      fill_min > n)
    return 2;
  const size_t px = (size_t)rows * cols;
  std::unique_ptr<uint8_t[]> disp_b, src_b, w_b, want_out, want_count, want_spread, want_flags, want_counts;
  if (!read_npy(dir + "disp.npy", 4 * px, &disp_b) || !read_npy(dir + "sources.npy", 4 * px * n, &src_b) ||
      !read_npy(dir + "weights.npy", 4 * px * (n + 1), &w_b) || !read_npy(dir + "want_out.npy", 4 * px, &want_out) ||
      !read_npy(dir + "want_count.npy", px, &want_count) || !read_npy(dir + "want_spread.npy", 4 * px, &want_spread) ||
      !read_npy(dir + "want_flags.npy", px, &want_flags) || !read_npy(dir + "want_counts.npy", 16, &want_counts))
    return 2;
  std::unique_ptr<float[]> disp(new float[px]);
  memcpy(disp.get(), disp_b.get(), 4 * px);
  std::unique_ptr<float[]> maps[pm::kFuseMaxSources], weights[pm::kFuseMaxSources + 1];  // exactly sized allocations
  auto plane = [&](const uint8_t* from) {
    std::unique_ptr<float[]> q(new float[px]);
    memcpy(q.get(), from, 4 * px);
    return q;
  };
  pm::FuseArgs a = {};
  a.cam = pm::cloud_cam(camera);
  a.rows = rows, a.cols = cols, a.n = n, a.px = px;
  a.max_diff = (float)p[9], a.min_consistent = (int)p[10], a.max_conflicts = (int)p[11];
  a.fill_min_sources = fill_min, a.fill_max_diff = (float)p[13];
  if (p[14] != 0.0) {
    weights[0] = plane(w_b.get());
    a.weight = weights[0].get();
  }
  pm::FuseSplatArgs sa = {};
  sa.cam = a.cam, sa.rows = rows, sa.cols = cols, sa.px = px;
  for (int k = 0; k < n; ++k) {
    maps[k] = plane(src_b.get() + 4 * px * k);
    const double* m = p + kHead + pm::kFuseMaxSources + 12 * k;
    const double *R = m, *t = m + 9;
    for (int i = 0; i < 9; ++i) a.src[k].R[i] = R[i];
    for (int i = 0; i < 3; ++i) a.src[k].t[i] = t[i];
    a.src[k].map = maps[k].get();
    if (p[kHead + k] != 0.0) {
      weights[k + 1] = plane(w_b.get() + 4 * px * (k + 1));
      a.src[k].weight = weights[k + 1].get();
    }
    for (int i = 0; i < 3; ++i) {  // the inverse motion, as pm_fuse_disparity forms it on the host
      for (int j = 0; j < 3; ++j) sa.src[k].R[3 * i + j] = R[3 * j + i];
      sa.src[k].t[i] = -(((R[i] * t[0]) + (R[3 + i] * t[1])) + (R[6 + i] * t[2]));
    }
    sa.src[k].map = maps[k].get();
  }
  int bad = 0;
  for (int pass = 0; pass < 4; ++pass) {  // forwards, backwards, in place, the counts alone
    const bool backwards = pass == 1;
    const char* const name = pass == 0 ? "forwards" : pass == 1 ? "backwards" : pass == 2 ? "in place" : "counts alone";
    std::unique_ptr<float[]> cur(new float[px]), out(new float[px]), spread(new float[px]);
    std::unique_ptr<uint8_t[]> count(new uint8_t[px]), flags(new uint8_t[px]);
    std::unique_ptr<unsigned[]> splat;  // no map scratch without a fill
    if (fill_min >= 1) {
      splat.reset(new unsigned[px * n]());
      sa.splat = splat.get();
      run_splat(sa, n, backwards);
    }
    memcpy(cur.get(), disp.get(), 4 * px);
    int counts[4] = {0, 0, 0, 0};
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
