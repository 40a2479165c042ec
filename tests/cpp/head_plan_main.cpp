// head_plan_main.cpp -- the plan of k_setup's launch (csrc/pm_head_plan.hpp) on a host alone, for a sanitizer run:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iocean-perception_amd/csrc
//       tests/cpp/head_plan_main.cpp -o head_plan_main && ./head_plan_main
// For the shapes of tests/test_head_stages.py, 1 .. 3 pairs, every view and both kinds of handle it checks what the
// launch relies on: the blocks 0 .. setup_blocks - 1 cover the (bx, by, z) box of every section exactly once -- no block
// is idle, no box is covered twice --, and the planes and slots of the two one-view launches are disjoint and add up to
// those of the launch for both views.  Exit status 0 = clean.
#include <cstdio>
#include <set>
#include <tuple>
#include <vector>

#include "pm_head_plan.hpp"

namespace {

long g_bad = 0;
void expect(bool ok, const char* what, int rows, int cols, int n, int view, int with_lines) {
  if (ok) return;
  if (g_bad++ < 20) std::fprintf(stderr, "%s: %dx%d n %d view %d with_lines %d\n", what, cols, rows, n, view, with_lines);
}

constexpr int kTransPad = 16;  // csrc/pm_device.hpp

using Place = std::tuple<int, int, int>;  // bx, by, z

}  // namespace

int main() {
  const int shapes[][2] = {{8, 8}, {8, 14}, {9, 15}, {64, 64}, {65, 65}, {66, 257}, {131, 70}, {5, 9}, {6, 8}, {7, 64}};
  long n_plans = 0;
  for (const auto& shape : shapes)
    for (int n = 1; n <= 3; ++n)
      for (int with_lines = 0; with_lines < 2; ++with_lines) {
        const int rows = shape[0], cols = shape[1], nrl = rows + 2, ncl = cols + kTransPad + 2;
        std::set<int> planes[3], slots[3];  // of view -1, 0, 1: index view + 1
        for (int view = -1; view <= 1; ++view) {
          const pm::SetupGrid sg = pm::setup_grid(rows, cols, nrl, ncl, n, view, with_lines);
          ++n_plans;
          // the box of every section: its sizes in blocks and the z values it must reach
          std::vector<int> want_planes, want_slots;
          for (int b = 0; b < n; ++b)
            for (int v = 0; v < 2; ++v) {
              if (view >= 0 && v != view) continue;
              want_slots.push_back(b * 2 + v);
              want_planes.push_back(b * 4 + 2 * v);
              want_planes.push_back(b * 4 + 2 * v + 1);
            }
          const int tiles_x = (cols + 63) / 64, tiles_y = (rows + 63) / 64;
          const int lines_x = (cols + 255) / 256, lines_y = (nrl + pm::kLinesPerSetupThread - 1) / pm::kLinesPerSetupThread;
          const int ctile_x = (ncl + 31) / 32;
          std::set<Place> want[pm::kSetupSections], got[pm::kSetupSections];
          for (int s = 0; s < pm::kSetupSections; ++s) {
            if (s >= pm::kSetupRowTriples && !with_lines) continue;
            const bool transpose = s < pm::kSetupRowTriples, col = s == pm::kSetupColTriples;
            const int nx = transpose ? tiles_x : col ? ctile_x : lines_x, ny = transpose || col ? tiles_y : lines_y;
            for (int z : transpose ? want_planes : want_slots)
              for (int by = 0; by < ny; ++by)
                for (int bx = 0; bx < nx; ++bx) want[s].insert(Place(bx, by, z));
          }
          // a section's blocks reach every pixel / line of its plane: tiles of 64 x 64, 256 x kLinesPerSetupThread, 32 x 64
          expect(tiles_x * 64 >= cols && tiles_y * 64 >= rows && lines_x * 256 >= cols &&
                     lines_y * pm::kLinesPerSetupThread >= nrl && ctile_x * 32 >= ncl,
                 "the boxes cover the planes", rows, cols, n, view, with_lines);
          const unsigned blocks = pm::setup_blocks(sg);
          size_t total = 0;
          for (const auto& w : want) total += w.size();
          expect(blocks == total, "as many blocks as places", rows, cols, n, view, with_lines);
          bool twice = false, section_ok = true;
          for (unsigned b = 0; b < blocks; ++b) {
            const pm::SetupBlock w = pm::setup_decode(sg, b);
            if (w.section < 0 || w.section >= pm::kSetupSections) {
              section_ok = false;
              continue;
            }
            twice |= !got[w.section].insert(Place(w.bx, w.by, w.z)).second;
            (w.section < pm::kSetupRowTriples ? planes : slots)[view + 1].insert(w.z);
          }
          expect(section_ok, "every block has a section", rows, cols, n, view, with_lines);
          expect(!twice, "no place is covered twice", rows, cols, n, view, with_lines);
          for (int s = 0; s < pm::kSetupSections; ++s)
            expect(got[s] == want[s], "a section's blocks cover its box exactly", rows, cols, n, view, with_lines);
        }
        for (const auto* sets : {planes, slots}) {
          std::set<int> both = sets[1];
          both.insert(sets[2].begin(), sets[2].end());
          expect(both.size() == sets[1].size() + sets[2].size(), "the two views' planes / slots are disjoint", rows, cols, n, 0,
                 with_lines);
          expect(both == sets[0], "... and add up to those of both views", rows, cols, n, -1, with_lines);
        }
        expect(with_lines ? slots[0].size() == (size_t)n * 2 : slots[0].empty(), "slots exist with the line planes only", rows,
               cols, n, -1, with_lines);
        expect(planes[0].size() == (size_t)n * 4, "four planes per pair", rows, cols, n, -1, with_lines);
      }
  std::printf("setup_grid: %ld plans, %ld broken\n", n_plans, g_bad);
  return g_bad ? 1 : 0;
}
