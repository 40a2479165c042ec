// sweep_plan_main.cpp -- plan_sweep (csrc/pm_sweep_plan.hpp) on a host alone, for a sanitizer run:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iocean-perception_amd/csrc
//       tests/cpp/sweep_plan_main.cpp -o sweep_plan_main && ./sweep_plan_main
// Walks shapes, windows, amplitudes, engines and slot counts -- the degenerate ones included: a chain of one position, one
// chain, 64 slots, chains either side of the LDS limit -- and checks what every launch relies on: a kernel the library
// holds, segments that cover the chain, a workgroup within the launch bounds, LDS within the CU's.  Exit status 0 = clean.
#include <cstdio>

#include "pm_sweep_plan.hpp"

namespace {

long g_bad = 0;
void expect(bool ok, const char* what, const pm::SweepVariant& v) {
  if (ok) return;
  if (g_bad++ < 20)
    std::fprintf(stderr, "%s: engine %d axis %d dir %d group %d waves %d window %d lref %d chain %d x %d seg %d lds %zu block %d\n",
                 what, v.engine, v.axis, v.dir, v.group, v.waves, v.window, v.lref, v.chain_len, v.chains, v.seg_len,
                 v.lds_bytes, v.block);
}

// the interior and the k-th sweep of an iteration, as csrc/pm_engine.hip::interior / sweep_geom
bool geometry(int sem, int rows, int cols, int pw, int ph, int k, pm::SweepGeom* g) {
  const bool cpu = sem == PM_SEM_CPU;
  const int x_lo = cpu ? pw / 2 : 1, x_hi = cpu ? cols - pw / 2 - 1 : cols - 2;
  const int y_lo = cpu ? ph / 2 : 1, y_hi = cpu ? rows - ph / 2 - 1 : rows - 2;
  g->axis = k & 1;
  g->dir = k < 2 ? 1 : -1;
  const int lo = g->axis == 0 ? x_lo : y_lo, hi = g->axis == 0 ? x_hi : y_hi;
  g->c_lo = g->axis == 0 ? y_lo : x_lo;
  g->c_hi = g->axis == 0 ? y_hi : x_hi;
  g->s_first = g->dir > 0 ? lo : hi;
  g->s_last = cpu ? (g->dir > 0 ? hi : lo) : (g->dir > 0 ? hi - 1 : lo + 1);
  return g->c_hi - g->c_lo + 1 > 0 && (g->s_last - g->s_first) * g->dir >= 0;
}

void check(int sem, int pw, int ph, const pm::SweepGeom& g, int slots, int engine, float amp, int rows, int cols) {
  const pm::SweepVariant v = pm::plan_sweep(sem, pw, ph, rows, cols, g, slots, engine, amp);
  expect(v.axis == g.axis && v.dir == g.dir && v.chain_len >= 1 && v.chains >= 1, "geometry", v);
  expect(v.lds_bytes <= pm::kChainLdsMax, "LDS beyond the CU's", v);
  if (v.engine == PM_ENGINE_SERIAL || v.engine == PM_ENGINE_WAVE) {
    expect(v.group == 0 && v.waves == 0 && v.window == 0 && v.lref == 0 && v.seg_len == 0 && v.block == pm::kWave,
           "an engine without segments", v);
    expect(v.engine == engine || (v.engine == PM_ENGINE_SERIAL && !(engine == PM_ENGINE_WAVE && sem == PM_SEM_CPU)),
           "engine", v);
    return;
  }
  expect(v.engine == PM_ENGINE_RUNBLK2 && (engine == PM_ENGINE_RUNBLK2 || engine == PM_ENGINE_AUTO), "engine", v);
  expect(v.waves >= 1 && v.waves <= pm::kMaxSegWaves && v.block == pm::kWave * v.waves, "workgroup", v);
  const int nseg = (pm::kWave / (v.group ? v.group : 1)) * v.waves;
  expect(v.seg_len >= 8 && (long long)v.seg_len * nseg >= v.chain_len, "segments do not cover the chain", v);
  if (sem == PM_SEM_CPU) {  // the instantiated k_runblk3 set (pm_sweeps.hip::launch_planned)
    const bool held = v.window == 0 ? v.group == 32
                                    : (v.window == 3 || v.window == 5) ? v.group == 16
                                                                       : (v.window == 7 || v.window == 9 || v.window == 11) &&
                                                                             (v.group == 16 || v.group == 32);
    expect(held && (!v.lref || v.window == 11), "no such k_runblk3", v);
  } else {
    expect((v.group == 8 || v.group == 16 || v.group == 32) && v.window == 0 && !v.lref, "no such k_runblk2", v);
  }
}

}  // namespace

int main() {
  const int sizes[] = {3, 4, 5, 11, 12, 13, 43, 64, 399, 400, 412, 922, 923, 1601, 1611, 2048, 2060, 8126, 8127, 10165, 10166, 20000};
  const int windows[][2] = {{3, 3}, {5, 5}, {7, 7}, {9, 9}, {11, 11}, {13, 13}, {3, 7}, {11, 3}, {15, 15}, {1, 1}};
  const float amps[] = {0.f, 0.5f, 0.50001f, 4.f, 8.f, 16.f, 16.5f, 1e30f};
  const int engines[] = {PM_ENGINE_AUTO, PM_ENGINE_SERIAL, PM_ENGINE_WAVE, PM_ENGINE_RUNBLK2};
  const int slot_counts[] = {1, 2, 64};
  long n = 0;
  for (int sem = PM_SEM_CPU; sem <= PM_SEM_GPU; ++sem)
    for (int rows : sizes)
      for (int cols : sizes)
        for (const auto& w : windows) {
          if (sem == PM_SEM_GPU && (w[0] != 3 || w[1] != 3)) continue;  // cost_params: its window is 3 x 3
          for (int k = 0; k < 4; ++k) {
            pm::SweepGeom g;
            if (!geometry(sem, rows, cols, w[0], w[1], k, &g)) continue;
            for (float amp : amps)
              for (int engine : engines)
                for (int slots : slot_counts) {
                  check(sem, w[0], w[1], g, slots, engine, amp, rows, cols);
                  ++n;
                }
          }
        }
  std::printf("plan_sweep: %ld plans, %ld broken\n", n, g_bad);
  return g_bad ? 1 : 0;
}
