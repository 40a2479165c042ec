// pm_tiled_steps.hpp -- the row-tiled mode's schedules, each planned ONCE: plan_tiled returns one attempt of a Match() over
// n bands as the flat list of steps a single-threaded driver enqueues, in that order.  pm_tiled.hip walks the list through
// its runtime layer, python/tiled.py::match_band takes its rank's steps from pm_tiled_steps (include/pm/patchmatch.h) and
// does them through its comm, tests/cpp/tiled_steps_main.cpp proves on a host alone what the exactness of the mode rests
// on.  Everything the protocol decides is decided here and nowhere else:
//   * the predecessor of a band in a sweep direction, and the successor that reads what it publishes;
//   * which buffer of a band's double-buffered `sent` pair a row is published into and taken from;
//   * that the band at position pos of the sweep direction (0 = the band without a predecessor) is final after exchange
//     round pos - 1, takes no row from round pos on, and that its predecessor publishes none for it;
//   * that only a band with a successor asks whether its row moved after the last one it published;
//   * where a taken row must be a copy, and where the reader marks it as consumed.
// What a step does NOT name follows from the band alone: the image rows (boundary_rows below) and whether a band's kernels
// can read a neighbour's row where it lies (topology and exchange mode: an execution-time question).
// No HIP header: this compiles with a host compiler alone.  No choice made here changes a result.
#pragma once

#include <vector>

#include "pm/patchmatch.h"

namespace pm {

using TiledStep = pm_tiled_step;

// halo rows of image data a band carries beyond its own where the image continues
inline int halo_rows(const pm_params& p) {
  if (p.semantics != PM_SEM_CPU) return 2;
  int ph = p.bg_patch_h;
  for (int i = 0; i < p.patchmatch_iters; ++i) ph = p.patch_h[i] > ph ? p.patch_h[i] : ph;
  return ph / 2 + 1;
}
// band k of n: rows split as evenly as possible, halo clipped to the image
inline void band_of(int k, int n, int rows, int halo, pm_tile* t, int* band_rows) {
  const int base = rows / n, rem = rows % n;
  t->global_rows = rows;
  t->own_row0 = k * base + (k < rem ? k : rem);
  t->own_rows = base + (k < rem ? 1 : 0);
  t->band_row0 = t->own_row0 - halo > 0 ? t->own_row0 - halo : 0;
  const int end = t->own_row0 + t->own_rows + halo < rows ? t->own_row0 + t->own_rows + halo : rows;
  *band_rows = end - t->band_row0;
}

// The image rows of a band that a vertical pass (1: down, 3: up) carries across its boundaries: `out` is the band's last
// own row in sweep direction -- what it publishes -- and `pred` the row in front of its first: the predecessor's `out`.
struct BoundaryRows {
  int out, pred;
};
inline BoundaryRows boundary_rows(const pm_tile& t, int pass) {
  const int first = t.own_row0, last = t.own_row0 + t.own_rows - 1;
  return pass == 1 ? BoundaryRows{last, first - 1} : BoundaryRows{first, last + 1};
}

// exchange rounds per vertical sweep of the speculative schedule: the band at position pos is final after round pos - 1, so
// n - 1 rounds are always enough -- what a negative or larger count means
inline int tiled_rounds(int n_bands, int rounds) { return rounds < 0 || rounds > n_bands - 1 ? n_bands - 1 : rounds; }

inline std::vector<TiledStep> plan_tiled(int n, int iterations, int schedule, int rounds) {
  std::vector<TiledStep> steps;
  int it = -1, pass = -1, round = -1;
  auto add = [&](int op, int band) -> TiledStep& {
    steps.push_back(TiledStep{op, band, it, pass, round, -1, -1, 0, 0});
    return steps.back();
  };
  auto all = [&](int op) {
    for (int j = 0; j < n; ++j) add(op, j);
  };
  int cur = 0;                          // the buffer of every band's `sent` pair that is in use
  std::vector<int> last((size_t)n, 0);  // the buffer a band published into last
  int down = 1;
  auto pos_of = [&](int j) { return down ? j : n - 1 - j; };    // 0 = the first band of the sweep direction
  auto at = [&](int pos) { return down ? pos : n - 1 - pos; };  // ... and back
  // band j's boundary row -> its sent[cur], for its successor (the last band's has no reader)
  auto publish = [&](int j) {
    TiledStep& s = add(PM_TILED_OP_PUBLISH, j);
    s.peer = pos_of(j) + 1 < n ? at(pos_of(j) + 1) : -1;
    s.buffer = last[(size_t)j] = cur;
  };
  // band j's stage `op` on its predecessor's sent[cur] (the first band has none: the stage runs without a row)
  auto take = [&](int op, int j, int copy, int done_behind_copy) {
    TiledStep& s = add(op, j);
    if (pos_of(j) == 0) return;
    s.peer = at(pos_of(j) - 1);
    s.buffer = cur;
    s.copy = copy;
    s.done_behind_copy = done_behind_copy;
  };
  all(PM_TILED_OP_BEGIN);
  for (it = 0; it < iterations; ++it) {
    all(PM_TILED_OP_NOISE);
    for (pass = 0; pass < 4; ++pass) {
      if (pass == 0 || pass == 2) {  // horizontal sweeps never leave the band
        all(PM_TILED_OP_SWEEP);
        continue;
      }
      down = pass == 1;
      if (schedule == PM_TILED_SCHEDULE_PIPELINED) {
        // The bands sweep IN ORDER: each stores its predecessor's final row in front of its chains, sweeps once and
        // publishes its own last row.  One buffer per vertical sweep: its reader of two sweeps ago has long been waited for.
        cur ^= 1;
        for (int pos = 0; pos < n; ++pos) {
          if (pos > 0) take(PM_TILED_OP_SET_ROW, at(pos), 0, 0);
          add(PM_TILED_OP_SWEEP, at(pos));
          if (pos + 1 < n) publish(at(pos));
        }
        continue;
      }
      // SPECULATIVE.  The guess: every band sweeps from the row its predecessor held BEFORE the sweep.  That row is compared
      // with the next one that arrives, so it must be a copy in the band's own memory, consumed as soon as it is copied.
      for (int j = 0; j < n; ++j) publish(j);
      for (int j = 0; j < n; ++j) {
        take(PM_TILED_OP_PRESWEEP, j, 1, 1);
        add(PM_TILED_OP_SWEEP, j);
      }
      // Round r hands a band the row its predecessor held after round r - 1.  The band at position pos is final after
      // round pos - 1: from round pos on it would receive the row it already has, restore nothing and re-sweep nothing, so
      // it leaves the rounds and its predecessor publishes nothing for it -- n (n - 1) / 2 band-rounds, not (n - 1)^2.
      for (int r = 0; r < tiled_rounds(n, rounds); ++r) {
        round = r;
        cur ^= 1;
        for (int j = 0; j < n; ++j)
          if (pos_of(j) + 1 < n && pos_of(j) + 1 > r) publish(j);
        for (int j = 0; j < n; ++j)
          if (pos_of(j) > r) take(PM_TILED_OP_EXCHANGE_ROUND, j, 0, 1);
      }
      // did my row move after the last one I published?  then my successor is stale.  Only a band that HAS a successor
      // asks: the last band's row is an image border nobody consumes.
      for (int j = 0; j < n; ++j)
        if (pos_of(j) + 1 < n) add(PM_TILED_OP_ROW_MOVED, j).buffer = last[(size_t)j];
      round = -1;
    }
    pass = -1;
  }
  it = -1;
  for (int j = 0; j < n; ++j) {
    add(PM_TILED_OP_BACKGROUND, j);
    add(PM_TILED_OP_FINISH, j);
  }
  return steps;
}

}  // namespace pm
