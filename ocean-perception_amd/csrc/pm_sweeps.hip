// pm_sweeps.hip -- directional sweeps: engine selection, tuning knobs and every sweep kernel instantiation
// (pm_sweeps.hpp).  PatchmatchGpu's PropagateRow / PropagateCol (patchmatch_gpu.cu:116-230) and Patchmatch::Propagate's
// four passes (patchmatch.cpp:248-311).
#include "pm_sweeps.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pm_serial.hpp"
#include "pm_wave.hpp"
#include "pm_run2.hpp"
#include "pm_run3.hpp"

namespace pm {
namespace {

// The one mapping from a planned variant to a kernel instantiation: what the switches below list is what the library
// holds.  Nothing is decided or computed here (pm_sweep_plan.hpp::plan_sweep did that).
constexpr int variant_key(int group, int axis, int window, int dir, bool lref) {
  return (((window * 64 + group) * 2 + axis) * 2 + (dir < 0 ? 1 : 0)) * 2 + (lref ? 1 : 0);
}
#define PM_RUN3(GS, AXIS, TP, DIR, LREF) \
  case variant_key(GS, AXIS, TP, DIR, LREF): launch(k_runblk3<GS, AXIS, TP, DIR, LREF>); break;
#define PM_RUN3_DIRS(GS, AXIS, TP, LREF) PM_RUN3(GS, AXIS, TP, 1, LREF) PM_RUN3(GS, AXIS, TP, -1, LREF)
#define PM_RUN3_AXIS(AXIS)                                            \
  PM_RUN3_DIRS(16, AXIS, 3, false) PM_RUN3_DIRS(16, AXIS, 5, false)   \
  PM_RUN3_DIRS(16, AXIS, 7, false) PM_RUN3_DIRS(32, AXIS, 7, false)   \
  PM_RUN3_DIRS(16, AXIS, 9, false) PM_RUN3_DIRS(32, AXIS, 9, false)   \
  PM_RUN3_DIRS(16, AXIS, 11, true) PM_RUN3_DIRS(16, AXIS, 11, false)  \
  PM_RUN3_DIRS(32, AXIS, 11, true) PM_RUN3_DIRS(32, AXIS, 11, false)  \
  PM_RUN3_DIRS(32, AXIS, 0, false)
#define PM_RUN2(GS, AXIS) \
  case variant_key(GS, AXIS, 0, 1, false): launch(k_runblk2<GS, AXIS>); break;

void launch_planned(const PlaneSet& ps, const CostParams& cp, const SweepGeom& g, int slots, const SweepVariant& v,
                    hipStream_t stream, const SweepHint& hint) {
  if (v.engine == PM_ENGINE_SERIAL) {
    hipLaunchKernelGGL(k_sweep_serial, dim3((unsigned)((v.chains + 63) / 64), 1, (unsigned)slots), dim3(v.block), 0, stream,
                       ps, cp, g);
    return;
  }
  if (v.engine == PM_ENGINE_WAVE) {
    launch_sweep_wave(ps, cp, g, slots, v.lds_bytes, stream);
    return;
  }
  // the run engines: one workgroup per chain; arg: the kernel's arguments behind (ps, cp, g)
  auto launch_chain = [&](auto kernel, auto... arg) {
    // (static LDS counts against the same limit as the dynamic part: the row +1 variants of k_runblk3 have some)
    allow_big_lds(kernel, v.lds_bytes + kRun3StaticLds);
    hipLaunchKernelGGL(kernel, dim3((unsigned)v.chains, 1, (unsigned)slots), dim3((unsigned)v.block), v.lds_bytes, stream,
                       ps, cp, g, arg...);
  };
  if (cp.semantics != PM_SEM_CPU) {
    auto launch = [&](auto kernel) { launch_chain(kernel, v.seg_len); };
    switch (variant_key(v.group, v.axis, 0, 1, false)) {
      PM_RUN2(8, 0) PM_RUN2(16, 0) PM_RUN2(32, 0) PM_RUN2(8, 1) PM_RUN2(16, 1) PM_RUN2(32, 1)
      default: abort();  // plan_sweep gives no other combination
    }
    return;
  }
  auto launch = [&](auto kernel) {
    const int seg_len = v.seg_len | (sweep_knobs().run3_dbg << 24);  // (PM_RUN3_DBG: the tuning build's timing switches)
    // the stop-bit plane is a row +1 sweep's alone, and only of a plane set that has one
    const bool row_fwd = v.axis == 0 && v.dir > 0 && ps.stops;
    const int mode = (hint.mode == kSegHintPlane && !row_fwd) ? kSegHintNone : hint.mode;
    const int hint_bits = (mode & 3) | ((hint.write_stops && row_fwd) ? kRun3WriteStops : 0) |
                          ((hint.stop_w < 0 ? 0 : (hint.stop_w > kRun3MaxStopWeight ? kRun3MaxStopWeight : hint.stop_w)) << 8);
    launch_chain(kernel, seg_len, hint_bits, hint.dbg_bounds, hint.dbg_chain
#ifdef PM_RUN3_STATS  // (its kernels take one more argument: the launch's slot of the per-chain log)
                 , run3_stats_slot(stream, v.axis, v.dir, v.group, v.chain_len, v.chains, v.waves)
#endif
    );
  };
  switch (variant_key(v.group, v.axis, v.window, v.dir, v.lref != 0)) {
    PM_RUN3_AXIS(0) PM_RUN3_AXIS(1)
    default: abort();  // plan_sweep gives no other combination
  }
}
#undef PM_RUN3
#undef PM_RUN3_DIRS
#undef PM_RUN3_AXIS
#undef PM_RUN2

}  // namespace

SweepVariant launch_sweep(const PlaneSet& ps, const CostParams& cp, const SweepGeom& g, int slots, int engine, float amp,
                          hipStream_t stream, const SweepHint& hint) {
  const SweepVariant v = plan_sweep(cp.semantics, cp.pw, cp.ph, ps.rows, ps.cols, g, slots, engine, amp);
  launch_planned(ps, cp, g, slots, v, stream, hint);
  return v;
}

}  // namespace pm

#ifdef PM_RUN3_STATS
// stats build only: start / stop the per-chain log, write it out.  File: "RUN3LOG1", launches, then per launch the host
// record (8 x int64: stream, axis, dir, gs, n, chains, waves, 0) and chains x 8 uint32 device words.
extern "C" __attribute__((visibility("default"))) int pm_run3_stats_enable(int on) {
  pm::run3_stats().on = on != 0;
  if (on) pm::run3_stats().recs.clear();
  return 0;
}
extern "C" __attribute__((visibility("default"))) int pm_run3_stats_dump(const char* path) {
  pm::Run3Stats& s = pm::run3_stats();
  if (hipDeviceSynchronize() != hipSuccess) return -3;
  FILE* f = fopen(path, "wb");
  if (!f) return -1;
  const long long nl = (long long)s.recs.size();
  fwrite("RUN3LOG1", 1, 8, f);
  fwrite(&nl, sizeof(nl), 1, f);
  std::vector<unsigned> buf;
  for (size_t i = 0; i < s.recs.size(); ++i) {
    const pm::Run3StatsRec& r = s.recs[i];
    const long long rec[8] = {(long long)r.stream, r.axis, r.dir, r.gs, r.n, r.chains, r.waves, 0};
    fwrite(rec, sizeof(rec), 1, f);
    buf.resize(8 * (size_t)r.chains);
    if (hipMemcpy(buf.data(), s.d_log + 8 * (size_t)pm::Run3Stats::kMaxChains * i, sizeof(unsigned) * buf.size(),
                  hipMemcpyDeviceToHost) != hipSuccess) {
      fclose(f);
      return -3;
    }
    fwrite(buf.data(), sizeof(unsigned), buf.size(), f);
  }
  fclose(f);
  return (int)nl;
}
#endif
