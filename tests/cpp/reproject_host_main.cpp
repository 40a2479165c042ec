// reproject_host_main.cpp -- runs pm_reproject_disparity's own per-thread code (csrc/pm_reproject_body.hpp:
// reproject_splat_lane, reproject_stage_cell, reproject_finish_pixel, reproject_right_lane -- the bodies of the kernels of
// csrc/pm_reproject.hpp) on the HOST, so that tests/test_reproject.py can hold it to the definition
// (tests/reproject_ref.py) without a GPU and under -fsanitize=address,undefined.  Every buffer is a heap allocation of
// EXACTLY the bytes the stage may touch, the LDS tile included, and the tile is poisoned in front of every block: a cell
// that is read without having been staged shows as a mismatch.  The launches -- the splats' grid and block are the body
// header's span_blocks() and kReprojectBlockX / Y, the finish's its tile, all walked by host_launch.hpp -- run twice, blocks
// and threads forwards and then backwards: the result must not depend on the order (only integer maximum and addition cross
// threads).  Compiled as HIP source with the host-only switch of hipcc and -ffp-contract=off.
//   reproject_host_main <dir>
// <dir> holds .npy dumps (host_npy.hpp: Case): params.npy (float64: rows, cols, fx, fy, cx, cy, baseline, R[9], t[3], min_disp,
// max_disp, close_radius, shift), disp.npy (float32 [rows][cols]) and the definition's results want_seed_l.npy,
// want_seed_r.npy (float32 [rows][cols]) and want_counts.npy (int32 [2]).  shift: the source map and both outputs start
// `shift` floats into their allocation.
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.

#include "host_launch.hpp"
#include "host_npy.hpp"
#include "pm_reproject_body.hpp"

enum { kRows, kCols, kFx, kFy, kCx, kCy, kBaseline, kMotion, kMinDisp = kMotion + 12, kMaxDisp, kCloseRadius, kShift, kParams };

// every thread of every block of a splat launch: lane l of a row's wavefront on pixels l, l + 64, l + 128, l + 192
template <typename Args, typename Body>
static void run_splat(const Args& a, int rows, int cols, bool backwards, Body body) {
  const pm::SpanBlocks grid = pm::span_blocks(rows, cols);
  for_blocks(grid.x, grid.y, 1, backwards, [&](int bx, int by, int) {
    for_threads(pm::kReprojectBlockX, pm::kReprojectBlockY, backwards, [&](int tx, int ty) {
      const int x = bx * pm::kReprojectSpan + tx, y = by * pm::kReprojectBlockY + ty;
      if (x < cols && y < rows) body(a, x, y);
    });
  });
}

// every block of k_reproject_finish: a thread per cell to stage, then a thread per pixel of the tile
static void run_finish(const pm::ReprojectFinishArgs& a, bool backwards) {
  const int gx = (a.cols + pm::kReprojectTileW - 1) / pm::kReprojectTileW;
  const int gy = (a.rows + pm::kReprojectTileH - 1) / pm::kReprojectTileH;
  std::unique_ptr<unsigned[]> tile(new unsigned[pm::kReprojectTileWords]);
  for_blocks(gx, gy, 1, backwards, [&](int bx, int by, int) {
    const int x0 = bx * pm::kReprojectTileW, y0 = by * pm::kReprojectTileH;
    for (int k = 0; k < pm::kReprojectTileWords; ++k) tile[k] = 0xFFFFFFFFu;  // poison: larger than any staged word
    for_threads(pm::kReprojectTileW + 2 * a.r, pm::kReprojectTileH + 2 * a.r, backwards,
                [&](int lx, int ly) { pm::reproject_stage_cell(a, tile.get(), lx, ly, x0, y0); });
    int sums[1] = {0};
    for_threads(pm::kReprojectTileW, pm::kReprojectTileH, backwards,
                [&](int tx, int ty) { sums[0] += pm::reproject_finish_pixel(a, tile.get(), x0, y0, tx, ty) ? 1 : 0; });
    flush_sums(a.count, sums, pm::reproject_add);
  });
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Case c(argv[1]);
  const std::vector<double> p = c.params(kParams);
  const int rows = (int)p[kRows], cols = (int)p[kCols], r = (int)p[kCloseRadius], shift = (int)p[kShift];
  const pm_cloud_camera camera = {p[kFx], p[kFy], p[kCx], p[kCy], p[kBaseline]};
  if (c.failed || rows < 1 || cols < 1 || r < 0 || r > pm::kReprojectMaxRadius || shift < 0) return 2;
  const size_t px = (size_t)rows * cols;
  const auto disp_b = c.raw("disp", 4 * px), want_l = c.raw("want_seed_l", 4 * px), want_r = c.raw("want_seed_r", 4 * px);
  const auto want_counts = c.raw("want_counts", 8);
  if (c.failed) return 2;
  // the source `shift` floats into an allocation with nothing behind it (operator new aligns to 16 bytes, like hipMalloc)
  std::unique_ptr<float[]> disp(new float[shift + px]);
  memcpy(disp.get() + shift, disp_b.get(), 4 * px);
  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const bool backwards = pass == 1;
    const char* const name = backwards ? "backwards" : "forwards";  // a mismatch names the pass it happened in
    std::unique_ptr<unsigned[]> splat_l(new unsigned[px]()), splat_r(new unsigned[px]());  // the memset
    std::unique_ptr<unsigned[]> seed_l(new unsigned[shift + px]), seed_r(new unsigned[shift + px]);
    for (int k = 0; k < shift; ++k) seed_l[k] = seed_r[k] = 0xA5A5A5A5u;
    int counts[2] = {0, 0};
    pm::ReprojectArgs a = {pm::cloud_cam(camera), {}, {}, (float)p[kMinDisp], (float)p[kMaxDisp], disp.get() + shift, rows, cols,
                           splat_l.get()};
    read_motion(&p[kMotion], a.R, a.t);
    run_splat(a, rows, cols, backwards, pm::reproject_splat_lane);
    run_finish(pm::ReprojectFinishArgs{splat_l.get(), seed_l.get() + shift, rows, cols, r, &counts[0]}, backwards);
    const pm::ReprojectRightArgs ra = {reinterpret_cast<const float*>(seed_l.get() + shift), rows, cols, splat_r.get()};
    run_splat(ra, rows, cols, backwards, pm::reproject_right_lane);
    run_finish(pm::ReprojectFinishArgs{splat_r.get(), seed_r.get() + shift, rows, cols, r, &counts[1]}, backwards);
    bad |= differ("seed_l", seed_l.get() + shift, want_l.get(), 4 * px, name);
    bad |= differ("seed_r", seed_r.get() + shift, want_r.get(), 4 * px, name);
    bad |= differ("counts", counts, want_counts.get(), 8, name);
    for (int k = 0; k < shift; ++k) bad |= seed_l[k] != 0xA5A5A5A5u || seed_r[k] != 0xA5A5A5A5u;
    // counting alone (no output map) reaches the same counts
    int only[2] = {0, 0};
    run_finish(pm::ReprojectFinishArgs{splat_l.get(), nullptr, rows, cols, r, &only[0]}, backwards);
    run_finish(pm::ReprojectFinishArgs{splat_r.get(), nullptr, rows, cols, r, &only[1]}, backwards);
    bad |= differ("counts without a map", only, want_counts.get(), 8, name);
  }
  return bad ? 1 : 0;
}
