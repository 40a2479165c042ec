// pm_sweep_plan.hpp -- which kernel variant a directional sweep runs, and with what launch configuration: ONE pure host
// function, plan_sweep.  pm_sweeps.hip launches from its result (launch_planned), pm_debug_sweep_plan
// (include/pm/testing.h) returns it without a device, tests/test_sweep_plan.py pins it.  No HIP header: this compiles
// with a host compiler alone (tests/cpp/sweep_plan_main.cpp).  No choice made here changes a result.
#pragma once

#include <cstdlib>

#include "pm/patchmatch.h"
#include "pm_seg_bounds.hpp"
#include "pm_sweep_defs.hpp"
#include "pm_tune.hpp"

namespace pm {

// What plan_sweep decided for one sweep launch.  Host-side only, no kernel sees it.
struct SweepVariant {
  int engine = 0;          // PM_ENGINE_*, after the serial fallback
  int axis = 0, dir = 0;
  int group = 0;           // lanes per chain segment; 0: the engine has no groups
  int waves = 0;           // wavefronts per chain; 0: the engine has no chain segments
  int window = 0;          // compiled-in window of k_runblk3; 0: the general kernel, and every other engine
  int lref = 0;            // 1: reference lines staged in LDS
  int chain_len = 0, chains = 0;
  int seg_len = 0;         // positions per chain segment (at least 8); 0: the engine has no chain segments
  size_t lds_bytes = 0;    // dynamic LDS of the launch
  int block = 0;           // threads per workgroup
};

// The A/B knobs of the sweeps: read once per process, and only by the tuning build (pm_tune.hpp); the shipped library
// has the defaults compiled in.  0 = "the rule below" where a default is 0.
struct SweepKnobs {
  int group;           // PM_RUNBLK_GROUP: lanes per segment, 8 / 16 / 32
  int gpu_group[2];    // PM_GPU_GROUP_FWD / _BWD: PM_SEM_GPU's lanes per segment (16)
  float g16_amp[2][2];  // PM_G16_ROW_AMP / _COL_AMP, PM_G16_ROW_AMP_NEG / _COL_AMP_NEG: [backward][axis], see plan_sweep
  int waves[2][2];     // PM_RUNBLK_WAVES, _ROW, _COL, _ROW16, _COL16: wavefronts per chain, [axis][group <= 16]
  int gpu_waves[2];    // PM_GPU_WAVES_FWD / _BWD: PM_SEM_GPU's wavefronts per chain
  int lref;            // PM_RUN2_LREF: staged reference lines, bit 0 = row sweeps, bit 1 = column sweeps (2)
  size_t lref_limit;   // PM_RUN2_LREF_KB: LDS budget per workgroup with staged lines (40 KB)
  int run3_dbg;        // PM_RUN3_DBG: timing experiments of k_runblk3 (bit 0 no steps, bit 1 no reference staging)
  int lds_extra_kb;    // PM_RUN3_LDS_EXTRA_KB: pads k_runblk3's allocation (how sensitive is the step to workgroups per CU?)

  static int env_int(const char* name, int dflt) {
    const char* e = pm::tune_env(name);
    return e ? atoi(e) : dflt;
  }
  static float env_float(const char* name, float dflt) {
    const char* e = pm::tune_env(name);
    return e ? (float)atof(e) : dflt;
  }
  SweepKnobs() {
    const int g = env_int("PM_RUNBLK_GROUP", 0);
    group = (g == 8 || g == 16 || g == 32) ? g : 0;
    gpu_group[0] = env_int("PM_GPU_GROUP_FWD", 16);
    gpu_group[1] = env_int("PM_GPU_GROUP_BWD", 16);
    g16_amp[0][0] = env_float("PM_G16_ROW_AMP", 0.5f);
    g16_amp[0][1] = env_float("PM_G16_COL_AMP", 4.0f);
    g16_amp[1][0] = env_float("PM_G16_ROW_AMP_NEG", 8.0f);
    g16_amp[1][1] = env_float("PM_G16_COL_AMP_NEG", 16.0f);
    const char* names[2][2] = {{"PM_RUNBLK_WAVES_ROW", "PM_RUNBLK_WAVES_ROW16"},
                               {"PM_RUNBLK_WAVES_COL", "PM_RUNBLK_WAVES_COL16"}};
    const char* both = pm::tune_env("PM_RUNBLK_WAVES");
    for (int a = 0; a < 2; ++a)
      for (int g16 = 0; g16 < 2; ++g16) {
        const char* e = pm::tune_env(names[a][g16]);
        if (!e && g16 == 1) e = pm::tune_env(names[a][0]);
        if (!e) e = both;
        const int x = e ? atoi(e) : 0;
        waves[a][g16] = x < 1 ? 0 : (x > kMaxSegWaves ? kMaxSegWaves : x);
      }
    gpu_waves[0] = env_int("PM_GPU_WAVES_FWD", 0);
    gpu_waves[1] = env_int("PM_GPU_WAVES_BWD", 0);
    lref = env_int("PM_RUN2_LREF", 2);
    lref_limit = (size_t)env_int("PM_RUN2_LREF_KB", 40) * 1024;
    run3_dbg = env_int("PM_RUN3_DBG", 0);
    lds_extra_kb = env_int("PM_RUN3_LDS_EXTRA_KB", 0);
  }
};
inline const SweepKnobs& sweep_knobs() {
  static const SweepKnobs k;  // initialised once, thread-safe
  return k;
}

// Which hint source each sweep class of a Match() iteration gives k_runblk3 for its segment boundaries
// (pm_seg_bounds.hpp), indexed by the pass: 0 = row +1, 1 = column +1, 2 = row -1, 3 = column -1.  Shipped: the row +1
// sweep reads the stop bits its predecessor of the previous iteration wrote; every other class keeps the equal split.
// Measured (profiles/segment_balance_ab.txt): with the run boundaries of the state they start from the
// row -1 launches do not get shorter and the column -1 launches get longer, the pre-pass costing more than the balance
// wins; the column +1 sweep loses already in the simulation (tools/segment_balance.py).
// PM_SEG_HINT (tuning build): a bit per pass, 1 = that class takes its source (row +1: the plane, the others: run
// boundaries).  -DPM_RUN3_NO_SEG_HINT compiles the pre-pass out of the kernel and all classes keep the equal split.

// the largest stop weight the kernel's 32-bit sums hold: lane * W with lane < 32, W <= 4095 * weight
constexpr int kRun3MaxStopWeight = 16383;
static_assert((long long)(kSegHintMaxSeg - 1) * ((long long)kSegHintMaxLen * (kRun3MaxStopWeight + 1)) + kSegHintMaxSeg < 0x7fffffffLL,
              "k_runblk3's boundary targets overflow");
struct SegHintModes {
  int pass[4];
  int stop_w;  // PM_SEG_STOP_W: 0 = a predicted stop weighs the positions of a run step (the rule), else this many
  SegHintModes() {
    const int w = SweepKnobs::env_int("PM_SEG_STOP_W", 0);
    stop_w = w < 0 ? 0 : (w > kRun3MaxStopWeight ? kRun3MaxStopWeight : w);
#ifdef PM_RUN3_NO_SEG_HINT
    const int bits = 0;
#else
    const int bits = SweepKnobs::env_int("PM_SEG_HINT", 1);
#endif
    const int source[4] = {kSegHintPlane, kSegHintRuns, kSegHintRuns, kSegHintRuns};
    for (int k = 0; k < 4; ++k) pass[k] = ((bits >> k) & 1) ? source[k] : kSegHintNone;
  }
};
inline const SegHintModes& seg_hint_modes() {
  static const SegHintModes m;
  return m;
}

// The hint of sweep `pass` of iteration `it` of a Match() (pm_engine.hip::view_op launches from it; pm_debug_match_sweep_hint
// returns it without a device).  A class takes its source (seg_hint_modes) only where the chains are long enough to pay
// for the pre-pass (seg_hint_pays).  The row +1 sweep reads the stop bits the same sweep of the previous iteration of the
// same call wrote for the same interior, i.e. the same window -- iteration 0 and a window change take the equal split --
// and writes them where the next iteration will read them.
inline SweepHint match_sweep_hint(const pm_params& p, int it, int pass, int chain_len) {
  SweepHint hint;
  const int mode = seg_hint_modes().pass[pass];
  if (mode == kSegHintNone || !seg_hint_pays(chain_len)) return hint;
  hint.stop_w = seg_hint_modes().stop_w;
  if (mode != kSegHintPlane) {
    hint.mode = mode;
    return hint;
  }
  const auto same_window = [&](int a, int b) { return p.patch_w[a] == p.patch_w[b] && p.patch_h[a] == p.patch_h[b]; };
  hint.mode = (it > 0 && same_window(it - 1, it)) ? kSegHintPlane : kSegHintNone;
  hint.write_stops = (it + 1 < p.patchmatch_iters && same_window(it + 1, it)) ? 1 : 0;
  return hint;
}

// ---- dynamic LDS of the chain kernels, one formula each -------------------------------------------------------------
// (chain_lds_bytes(n, 4 * kMaxSegWaves + 4, planes), the serial fallback's estimate in plan_sweep, is deliberately
// conservative: it bounds all of them for any segment count.)
// k_runblk3: one float4 per position and the pixel before the chain, [nseg + 1] last values, [nseg] candidates, 2 flags
inline size_t run3_lds_bytes(int n, int nseg) { return sizeof(float) * (4 * (size_t)(n + 1) + 2 * (size_t)nseg + 3); }
// ... plus its staged reference lines (LREF): kLref4Stride dwords per image row (column sweeps) / column (row sweeps)
// ... and, outside this formula, kRun3StaticLds (pm_seg_bounds.hpp) bytes of STATIC LDS in the row +1 variants (the staged stop masks of
// pm_run3.hpp: one 64-bit word per 64 positions of the longest hinted chain).  kChainLdsMax leaves 1 KB below the CU's
// 160 KB for it; launch_planned counts it when it raises a kernel's LDS limit.
static_assert(kChainLdsMax + kRun3StaticLds <= 160 * 1024, "k_runblk3's static LDS does not fit beside the longest chain");
inline size_t run3_lref_bytes(int lines) { return sizeof(unsigned) * (size_t)kLref4Stride * lines; }
// k_runblk2: five planes (the fifth: what a position does with its predecessor's old value), [nseg + 1] last values, 2 flags
inline size_t run2_lds_bytes(int n, int nseg) { return chain_lds_bytes(n, nseg + 3, 5); }
// k_sweep_gpu_lanes: four planes, one last value per lane and the pixel before the chain
inline size_t wave_gpu_lds_bytes(int n) { return chain_lds_bytes(n, kWave + 1, 4); }

constexpr int kShortChain = 400, kManyChains = 2048;

// The variant of one directional sweep of `slots` slots.  pw x ph: the window (cost_params: 3 x 3 for PM_SEM_GPU);
// rows, cols: the PlaneSet's (they bound the staged reference lines only); engine = pm_params.engine; amp = the noise
// amplitude of the iteration.  g must hold a chain: at least one chain of at least one position.
inline SweepVariant plan_sweep(int semantics, int pw, int ph, int rows, int cols, const SweepGeom& g, int slots, int engine,
                               float amp) {
  const SweepKnobs& k = sweep_knobs();
  const bool cpu = semantics == PM_SEM_CPU;
  SweepVariant v;
  v.axis = g.axis, v.dir = g.dir;
  v.chains = g.c_hi - g.c_lo + 1;
  v.chain_len = (g.s_last - g.s_first) * g.dir + 1;
  const int n = v.chain_len;

  // ---- engine.  PM_SEM_GPU has two parallel engines: lane-per-segment (WAVE) and the shared-tap run step (RUNBLK2).
  // The chain engines hold a chain in LDS: beyond the CU's capacity only the serial engine remains.
  if (engine == PM_ENGINE_AUTO) engine = PM_ENGINE_RUNBLK2;
  if (engine != PM_ENGINE_SERIAL && !(engine == PM_ENGINE_WAVE && cpu) &&
      chain_lds_bytes(n, 4 * kMaxSegWaves + 4, cpu ? 4 : 5) > kChainLdsMax)
    engine = PM_ENGINE_SERIAL;
  v.engine = engine;
  v.block = kWave;
  if (engine == PM_ENGINE_SERIAL) return v;
  if (engine == PM_ENGINE_WAVE) {
    if (!cpu) v.lds_bytes = wave_gpu_lds_bytes(n);
    return v;
  }

  // ---- lanes per chain segment (32 or 16; PM_SEM_GPU also 8); PM_RUNBLK_GROUP overrides.  Measured
  // (tools/sweep_group.sh, 720p): PM_SEM_GPU's 3-lane window wins with 16-lane groups (1.60 vs 1.93 ms per
  // frame), PM_SEM_CPU's 11-lane window with 32 (a 16-lane strip leaves it only 5-6 positions per step).
  // Runs of adopted values get shorter as the noise amplitude decays, and short runs waste most of a 32-lane strip:
  // measured at 720p / 11x11 / amp 32/2^i (tools/sweep_waves.sh) column sweeps win with 16-lane groups from amplitude 4
  // on, row sweeps (one position fewer per strip: the DPP spare lane) only from 0.5 on.  That holds for the FORWARD
  // sweeps, which come first after the noise and carry a good value a long way; the BACKWARD sweeps of the same
  // iteration meet what the forward ones left -- short runs, 58 % more steps per launch
  // (profiles/r02d_pmc_insts.txt) -- and win with 16-lane groups from amplitude 8 (rows) / 16 (columns) on: 294 -> 307
  // pairs/s (tools/sweep_neg.sh, profiles/r02f_sweep_group_thresholds.txt).  Small windows leave 11+ positions in a
  // 16-lane strip: 16 wins at every amplitude.
  const int back = g.dir < 0 ? 1 : 0;
  int group = k.group;
  if (!group) {
    if (!cpu) group = k.gpu_group[back];
    else if ((g.axis == 0 ? pw : ph) <= 5) group = 16;
    else group = amp <= k.g16_amp[back][g.axis] ? 16 : 32;
  }

  // ---- wavefronts per chain: 4 up to ~1600 positions per chain, 8 beyond (measured: 720p best at 4,
  // tools/sweep_group.sh; 4096x2160 38.7 ms per frame at 8 vs 42.6 at 4), 2 for chains shorter than 400 positions --
  // the column chains of a 270-row band of a row-tiled 4096x2160 image: 8 / 16 segments of 17-35 positions are mostly
  // speculation boundaries (round 5: eight bands on one device 51.0 -> 48.4 ms in the tuning build) -- but only where
  // the launch has chains enough to fill the chip without them: the 376 x 240 pair of the reference's own test is
  // short chains on an EMPTY chip, and two wavefronts per chain took its call from 0.65 to 0.79 ms.
  int waves = cpu ? 0 : k.gpu_waves[back];
  if (!waves) waves = k.waves[g.axis][group <= 16 ? 1 : 0];
  if (!waves) waves = n > 1600 ? 8 : ((n < kShortChain && v.chains * slots >= kManyChains) ? 2 : 4);
  v.waves = waves < 1 ? 1 : (waves > kMaxSegWaves ? kMaxSegWaves : waves);

  // ---- the kernel.  PM_SEM_CPU: k_runblk3 with a compiled-in square window of 3 .. 11; windows of 3 and 5 always take
  // 16 lanes, windows the fixed-size kernels do not cover (not square, or wider than 11) the general kernel with 32.
  // Column sweeps of the benchmark window stage their reference lines in LDS (LREF) while that leaves room for at
  // least four workgroups per CU.  PM_SEM_GPU: k_runblk2.
  size_t lref_bytes = 0;
  if (cpu) {
    const int sq = pw == ph ? pw : 0;
    v.window = (sq == 3 || sq == 5 || sq == 7 || sq == 9 || sq == 11) ? sq : 0;
    v.group = v.window == 0 ? 32 : (v.window <= 5 ? 16 : (group <= 16 ? 16 : 32));
    if (v.window == 11 && ((k.lref >> g.axis) & 1)) {
      lref_bytes = run3_lref_bytes(g.axis == 1 ? rows : cols);
      if (run3_lds_bytes(n, 64) + lref_bytes <= k.lref_limit) v.lref = 1;
      else lref_bytes = 0;
    }
  } else {
    v.group = group <= 8 ? 8 : (group <= 16 ? 16 : 32);
  }
  const int nseg = (kWave / v.group) * v.waves;
  v.lds_bytes = cpu ? run3_lds_bytes(n, nseg) + lref_bytes + (size_t)k.lds_extra_kb * 1024 : run2_lds_bytes(n, nseg);
  v.seg_len = (n + nseg - 1) / nseg;
  if (v.seg_len < 8) v.seg_len = 8;
  v.block = kWave * v.waves;
  return v;
}

}  // namespace pm
