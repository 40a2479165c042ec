// pm_sweep_defs.hpp -- constants and types shared by the sweep kernels (pm_sweeps.hip), the host function that plans
// their launches (pm_sweep_plan.hpp) and their caller (pm_engine.hip).  No HIP here: the plan compiles on a host alone.
#pragma once

#include <cstddef>

namespace pm {

constexpr int kWave = 64;  // CDNA4 wavefront
constexpr int kMaxSegWaves = 16;  // wavefronts per chain of the run engines, at most
constexpr int kLref4Stride = 7;  // dwords per image row of the column sweeps' staged reference bytes (odd; 6 measures the same)

// The chain engines keep a whole chain (4 floats per position) in LDS.  Up to 64 KB of dynamic LDS is available
// by default; beyond that the kernel needs its limit raised (160 KB per CU on gfx950: chains of up to ~10 000
// positions).  plan_sweep falls back to the serial engine for longer chains.
constexpr size_t kChainLdsMax = 160 * 1024 - 1024;
inline size_t chain_lds_bytes(int n, int extra_words, int planes = 4) {
  const int n1 = (n + 1 + 3) & ~3;
  return sizeof(float) * ((size_t)planes * (size_t)n1 + (size_t)extra_words);
}

struct SweepGeom {
  int axis;           // 0 = along a row, 1 = along a column
  int dir;            // +1 / -1
  int c_lo, c_hi;     // chains (inclusive)
  int s_first, s_last;  // first and last visited position along the chain (inclusive)
};

// What a caller tells k_runblk3 about its segment boundaries (pm_seg_bounds.hpp).  The default is the equal split, which
// is what every caller outside Match()'s iterations launches.  Other engines ignore it.
struct SweepHint {
  int mode = 0;             // SegHint: where the predicted stops come from
  int write_stops = 0;      // 1: a row +1 sweep stores its stop bits into PlaneSet::stops for the next iteration
  int stop_w = 0;           // 0: a predicted stop weighs the positions of a run step (the rule); else this many (tuning)
  int* dbg_bounds = nullptr;  // device, [segments + 1]: the boundaries chain dbg_chain of slot 0 used (test hook)
  int dbg_chain = -1;
};

}  // namespace pm
