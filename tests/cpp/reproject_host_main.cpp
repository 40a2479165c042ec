// reproject_host_main.cpp -- runs pm_reproject_disparity's own per-thread code (csrc/pm_reproject_body.hpp:
// reproject_splat_lane, reproject_stage_cell, reproject_finish_pixel, reproject_right_lane -- the bodies of the kernels of
// csrc/pm_reproject.hpp) on the HOST, so that tests/test_reproject.py can hold it to the definition
// (tests/reproject_ref.py) without a GPU and under -fsanitize=address,undefined.  Every buffer is a heap allocation of
// EXACTLY the bytes the stage may touch, the LDS tile included, and the tile is poisoned in front of every block: a cell
// that is read without having been staged shows as a mismatch.  The launches run twice, blocks and threads forwards and
// then backwards: the result must not depend on the order (only integer maximum and addition cross threads).  Compiled as
// HIP source with the host-only switch of hipcc and -ffp-contract=off.
//   reproject_host_main <dir>
// <dir> holds .npy dumps (numpy's format, version 1, C order, little endian; the header is skipped and the payload size
// checked): params.npy (float64: rows, cols, fx, fy, cx, cy, baseline, R[9], t[3], min_disp, max_disp, close_radius, shift),
// disp.npy (float32 [rows][cols]) and the definition's results want_seed_l.npy, want_seed_r.npy (float32 [rows][cols]) and
// want_counts.npy (int32 [2]).  shift: the source map and both outputs start `shift` floats into their allocation.
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "host_npy.hpp"
#include "pm_reproject_body.hpp"

// a mismatch names the pass it happened in
static int differ_pass(const char* what, bool backwards, const void* got, const void* want, size_t bytes) {
  return differ(what, got, want, bytes, backwards ? "backwards" : "forwards");
}

// i-th of n, counted from the front or from the back
static int nth(int i, int n, bool backwards) { return backwards ? n - 1 - i : i; }

// every thread of a splat launch: a wavefront per 256 pixels of a row, lane l on pixels l, l + 64, l + 128, l + 192
template <typename Args, typename Body>
static void run_splat(const Args& a, int rows, int cols, bool backwards, Body body) {
  const int span = pm::kReprojectLanes * pm::kReprojectPixelsPerLane;
  const int waves = (cols + span - 1) / span;
  for (int j = 0; j < rows; ++j)
    for (int i = 0; i < waves * pm::kReprojectLanes; ++i) {
      const int t = nth(i, waves * pm::kReprojectLanes, backwards);
      const int x = (t / pm::kReprojectLanes) * span + t % pm::kReprojectLanes;
      if (x < cols) body(a, x, nth(j, rows, backwards));
    }
}

// every block of k_reproject_finish
static void run_finish(const pm::ReprojectFinishArgs& a, bool backwards) {
  const int gx = (a.cols + pm::kReprojectTileW - 1) / pm::kReprojectTileW;
  const int gy = (a.rows + pm::kReprojectTileH - 1) / pm::kReprojectTileH;
  std::unique_ptr<unsigned[]> tile(new unsigned[pm::kReprojectTileWords]);
  for (int b = 0; b < gx * gy; ++b) {
    const int block = nth(b, gx * gy, backwards);
    const int x0 = (block % gx) * pm::kReprojectTileW, y0 = (block / gx) * pm::kReprojectTileH;
    for (int k = 0; k < pm::kReprojectTileWords; ++k) tile[k] = 0xFFFFFFFFu;  // poison: larger than any staged word
    const int w = pm::kReprojectTileW + 2 * a.r, cells = w * (pm::kReprojectTileH + 2 * a.r);
    for (int i = 0; i < cells; ++i) {
      const int c = nth(i, cells, backwards);
      pm::reproject_stage_cell(a, tile.get(), c % w, c / w, x0, y0);
    }
    int sum = 0;
    const int threads = pm::kReprojectTileW * pm::kReprojectTileH;
    for (int i = 0; i < threads; ++i) {
      const int t = nth(i, threads, backwards);
      sum += pm::reproject_finish_pixel(a, tile.get(), x0, y0, t % pm::kReprojectTileW, t / pm::kReprojectTileW) ? 1 : 0;
    }
    if (sum) pm::reproject_add(a.count, sum);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = std::string(argv[1]) + "/";
  std::unique_ptr<uint8_t[]> raw;
  if (!read_npy(dir + "params.npy", 23 * sizeof(double), &raw)) return 2;
  double p[23];
  memcpy(p, raw.get(), sizeof p);
  const int rows = (int)p[0], cols = (int)p[1], r = (int)p[21], shift = (int)p[22];
  const pm_cloud_camera camera = {p[2], p[3], p[4], p[5], p[6]};
  if (rows < 1 || cols < 1 || r < 0 || r > pm::kReprojectMaxRadius || shift < 0) return 2;
  const size_t px = (size_t)rows * cols;
  std::unique_ptr<uint8_t[]> disp_b, want_l, want_r, want_counts;
  if (!read_npy(dir + "disp.npy", 4 * px, &disp_b) || !read_npy(dir + "want_seed_l.npy", 4 * px, &want_l) ||
      !read_npy(dir + "want_seed_r.npy", 4 * px, &want_r) || !read_npy(dir + "want_counts.npy", 8, &want_counts))
    return 2;
  // the source `shift` floats into an allocation with nothing behind it (operator new aligns to 16 bytes, like hipMalloc)
  std::unique_ptr<float[]> disp(new float[shift + px]);
  memcpy(disp.get() + shift, disp_b.get(), 4 * px);
  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const bool backwards = pass == 1;
    std::unique_ptr<unsigned[]> splat_l(new unsigned[px]()), splat_r(new unsigned[px]());  // the memset
    std::unique_ptr<unsigned[]> seed_l(new unsigned[shift + px]), seed_r(new unsigned[shift + px]);
    for (int k = 0; k < shift; ++k) seed_l[k] = seed_r[k] = 0xA5A5A5A5u;
    int counts[2] = {0, 0};
    pm::ReprojectArgs a = {pm::cloud_cam(camera), {}, {}, (float)p[19], (float)p[20], disp.get() + shift, rows, cols, splat_l.get()};
    for (int i = 0; i < 9; ++i) a.R[i] = p[7 + i];
    for (int i = 0; i < 3; ++i) a.t[i] = p[16 + i];
    run_splat(a, rows, cols, backwards, pm::reproject_splat_lane);
    run_finish(pm::ReprojectFinishArgs{splat_l.get(), seed_l.get() + shift, rows, cols, r, &counts[0]}, backwards);
    const pm::ReprojectRightArgs ra = {reinterpret_cast<const float*>(seed_l.get() + shift), rows, cols, splat_r.get()};
    run_splat(ra, rows, cols, backwards, pm::reproject_right_lane);
    run_finish(pm::ReprojectFinishArgs{splat_r.get(), seed_r.get() + shift, rows, cols, r, &counts[1]}, backwards);
    bad |= differ_pass("seed_l", backwards, seed_l.get() + shift, want_l.get(), 4 * px);
    bad |= differ_pass("seed_r", backwards, seed_r.get() + shift, want_r.get(), 4 * px);
    bad |= differ_pass("counts", backwards, counts, want_counts.get(), 8);
    for (int k = 0; k < shift; ++k) bad |= seed_l[k] != 0xA5A5A5A5u || seed_r[k] != 0xA5A5A5A5u;
    // counting alone (no output map) reaches the same counts
    int only[2] = {0, 0};
    run_finish(pm::ReprojectFinishArgs{splat_l.get(), nullptr, rows, cols, r, &only[0]}, backwards);
    run_finish(pm::ReprojectFinishArgs{splat_r.get(), nullptr, rows, cols, r, &only[1]}, backwards);
    bad |= differ_pass("counts without a map", backwards, only, want_counts.get(), 8);
  }
  return bad ? 1 : 0;
}
