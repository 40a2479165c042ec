// planes_plan_main.cpp -- plan_planes (csrc/pm_planes_plan.hpp) on a host alone, for a sanitizer run:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iocean-perception_amd/csrc
//       tests/cpp/planes_plan_main.cpp -o planes_plan_main && ./planes_plan_main
// Walks stages, windows, window shapes, state types, disparity ranges, view counts and image sizes -- 1 x 1 and sizes either
// side of every tile edge included -- and checks what every launch relies on: a grid that covers the image, a workgroup
// of one wavefront per tile row, LDS that holds what the kernel lays out in it, the fast fill only where its loads are
// whole dwords and its strips cover the tile row, and the all-zero record exactly where nothing runs.  Exit status 0 = clean.
#include <cmath>
#include <cstdio>

#include "pm_planes_plan.hpp"

namespace {

long g_bad = 0;
void expect(bool ok, const char* what, const pm::PlanesVariant& v, int rows, int cols, int max_disp) {
  if (ok) return;
  if (g_bad++ < 20)
    std::fprintf(stderr, "%s: stage %d P %d window %d f16 %d tile %dx%d grid %dx%d lds %d rw %d margin %d fast %d regs %d taps %d "
                         "(image %dx%d, max_disp %d)\n",
                 what, v.stage, v.patch, v.window, v.state_f16, v.tile_w, v.tile_h, v.grid_x, v.grid_y, v.lds_bytes, v.rw,
                 v.margin, v.fast_fill, v.ref_regs, v.tap_class, cols, rows, max_disp);
}

}  // namespace

int main() {
  const int sizes[] = {1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 130, 131, 257, 1280};
  const int disps[] = {1, 16, 20, 21, 128, 347, 348, 411, 412, 1024};
  long n = 0;
  for (int stage = pm::PL_INIT; stage <= pm::PL_VIEW_REFINE; ++stage)
    for (int P = 3; P <= 15; P += 2)
      for (int window = 0; window <= 1; ++window)
        for (int f16 = 0; f16 <= 1; ++f16)
          for (int nv = 1; nv <= 2; ++nv)
            for (int md : disps)
              for (int rows : sizes)
                for (int cols : sizes)
                  for (int aligned = 0; aligned <= 1; ++aligned) {
                    pm::PlanesParams pp{};
                    pp.patch = P;
                    pp.max_disp = md;
                    pp.slope_max = 1.0f;
                    pp.margin = (int)std::ceil(2.0 * (P / 2) * 1.0) + 2;
                    pp.window = window;
                    pp.n_views = nv;
                    const pm::PlanesVariant v = pm::plan_planes(pp, f16 != 0, stage, rows, cols, aligned != 0);
                    ++n;
                    if (stage == pm::PL_VIEW && nv == 1) {
                      expect(!v.launched && !v.stage && !v.patch && !v.tile_w && !v.grid_x && !v.lds_bytes && !v.rw &&
                                 !v.fast_fill && !v.ref_regs && !v.tap_class, "a no-op with a record", v, rows, cols, md);
                      continue;
                    }
                    const int ran = (stage == pm::PL_VIEW_REFINE && nv == 1) ? pm::PL_REFINE : stage;
                    expect(v.launched == 1 && v.stage == ran && v.patch == P && v.window == window && v.state_f16 == f16,
                           "variant", v, rows, cols, md);
                    expect(v.tile_w == pm::pl_tile_w(ran) && v.tile_h == pm::pl_tile_h(ran) && v.tile_h >= 1 && v.tile_h <= 16,
                           "tile", v, rows, cols, md);
                    expect((long)v.grid_x * v.tile_w >= cols && (long)(v.grid_x - 1) * v.tile_w < cols &&
                               (long)v.grid_y * v.tile_h >= rows && (long)(v.grid_y - 1) * v.tile_h < rows,
                           "the grid does not cover the image exactly", v, rows, cols, md);
                    // every column a window of the tile can read: the tile, the window, the disparities, the slopes
                    expect(v.rw >= v.tile_w + (P - 1) + md + 2 * pp.margin + 1, "target row too short", v, rows, cols, md);
                    const long tr = v.tile_h + P - 1, lw = v.tile_w + P - 1;
                    const long ref_bytes = 2 * (window ? 2 : 1) * 4 * tr * 4 * pm::pl_ref_row_dwords((int)lw, window);
                    const long pl_bytes = ran == pm::PL_SPATIAL ? 3L * 4 * (v.tile_h + 2) * (v.tile_w + 2) : 0;
                    expect(v.lds_bytes >= ref_bytes + 8 * tr * v.rw + pl_bytes, "LDS below the kernel's layout", v, rows, cols, md);
                    expect(!v.fast_fill || ((cols & 1) == 0 && aligned && v.rw + 1 <= 128 * pm::kPlFillStrips),
                           "fast fill where it cannot run", v, rows, cols, md);
                    expect(v.fast_fill == (int)pm::pl_fast_fill(cols, v.rw, aligned != 0), "fast fill differs from its predicate",
                           v, rows, cols, md);
                    expect(v.ref_regs == 0 || (ran == pm::PL_SPATIAL && window == 1 && (P == 3 || P == 11)), "register window", v,
                           rows, cols, md);
                  }
  // what the record refuses
  pm::PlanesParams pp{};
  pp.patch = 4;
  pp.max_disp = 16;
  pp.n_views = 2;
  if (pm::plan_planes(pp, false, pm::PL_INIT, 8, 8, true).launched) ++g_bad;
  pp.patch = 11;
  if (pm::plan_planes(pp, false, 5, 8, 8, true).launched || pm::plan_planes(pp, false, pm::PL_INIT, 0, 8, true).launched) ++g_bad;
  std::printf("plan_planes: %ld plans, %ld broken\n", n, g_bad);
  return g_bad ? 1 : 0;
}
