// normals_fit_host_main.cpp -- runs pm_disparity_normals' own code (csrc/pm_normals_fit_body.hpp: normals_fit_stage,
// normals_fit_pixel<R>, normals_fit_store -- what every thread of k_normals_fit<R> runs) on the HOST, so that
// tests/test_normals_fit.py can hold it to the definition (tests/normals_fit_ref.py) without a GPU and under
// -fsanitize=address,undefined.  The map is walked tile by tile as the launch grid walks it; every tile is a heap allocation
// of EXACTLY the floats a workgroup's LDS tile has at that radius, filled by the kernel's staging function, and every output
// an allocation of exactly its bytes: a tap outside the staged halo, or a store outside the image, is reported.  Compiled
// as HIP source with the host-only switch of hipcc and -ffp-contract=off.
//   normals_fit_host_main <dir>
// <dir> holds .npy dumps (host_npy.hpp: Case): params.npy (float64: rows, cols, fx, fy, cx, cy, baseline, radius, max_diff,
// min_support, shift), disp.npy (float32 [rows][cols]) and the definition's want_normals.npy (float32 [rows][cols][3]),
// want_planes.npy (float32 [3][rows][cols]), want_support.npy (uint8 [rows][cols]).  shift: d_normals starts `shift` floats
// into its allocation.
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.

#include "host_npy.hpp"
#include "pm_normals_fit_body.hpp"

enum { kRows, kCols, kFx, kFy, kCx, kCy, kBaseline, kRadius, kMaxDiff, kMinSupport, kShift, kParams };

// the grid of k_normals_fit<R>, workgroup by workgroup, thread by thread
template <int R>
static void run(const pm::NormalsFitArgs& a) {
  constexpr int pitch = pm::normals_fit_tile_pitch(R);
  for (int y0 = 0; y0 < a.rows; y0 += pm::kNormalsFitTileRows)
    for (int x0 = 0; x0 < a.cols; x0 += pm::kNormalsFitTileCols) {
      std::unique_ptr<float[]> tile(new float[pm::normals_fit_tile_cells(R)]);
      pm::normals_fit_stage(tile.get(), R, a.disp, a.rows, a.cols, x0, y0, 0, 1);
      for (int ty = 0; ty < pm::kNormalsFitTileRows && y0 + ty < a.rows; ++ty)
        for (int tx = 0; tx < pm::kNormalsFitTileCols && x0 + tx < a.cols; ++tx) {
          const float* centre = tile.get() + (ty + R) * pitch + tx + R;
          pm::normals_fit_store(a, x0 + tx, y0 + ty, pm::normals_fit_pixel<R>(centre, pitch, R, a.max_diff, a.min_support));
        }
    }
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Case c(argv[1]);
  const std::vector<double> p = c.params(kParams);
  const int rows = (int)p[kRows], cols = (int)p[kCols], radius = (int)p[kRadius], min_support = (int)p[kMinSupport], shift = (int)p[kShift];
  const pm_cloud_camera camera = {p[kFx], p[kFy], p[kCx], p[kCy], p[kBaseline]};
  const float max_diff = (float)p[kMaxDiff];
  if (c.failed || rows < 1 || cols < 1 || radius < 1 || radius > pm::kNormalsFitMaxRadius || shift < 0) return 2;
  const size_t px = (size_t)rows * cols;
  const auto disp = c.read<float>("disp", px);
  const auto want_normals = c.raw("want_normals", 12 * px), want_planes = c.raw("want_planes", 12 * px);
  const auto want_support = c.raw("want_support", px);
  if (c.failed) return 2;
  std::unique_ptr<float[]> normals(new float[shift + 3 * px]), planes(new float[3 * px]);
  std::unique_ptr<uint8_t[]> support(new uint8_t[px]);
  for (int k = 0; k < shift; ++k) normals[k] = -77.f;
  const pm::NormalsFitArgs a = {pm::cloud_cam(camera), disp.get(), rows, cols, radius, max_diff, min_support, normals.get() + shift,
                                planes.get(),          support.get()};
  switch (radius) {
    case 1: run<1>(a); break;
    case 2: run<2>(a); break;
    case 3: run<3>(a); break;
    case 4: run<4>(a); break;
    case 5: run<5>(a); break;
    case 6: run<6>(a); break;
    default: run<7>(a); break;
  }
  int bad = 0;
  bad |= differ("normals", normals.get() + shift, want_normals.get(), 12 * px);
  bad |= differ("planes", planes.get(), want_planes.get(), 12 * px);
  bad |= differ("support", support.get(), want_support.get(), px);
  for (int k = 0; k < shift; ++k) bad |= normals[k] != -77.f;
  return bad ? 1 : 0;
}
