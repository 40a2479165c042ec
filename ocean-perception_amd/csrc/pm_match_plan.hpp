// pm_match_plan.hpp -- which launches of a Match() go onto which stream: ONE pure host function, plan_match.  The engine
// (pm_engine.hip, pm_hostpath.hip, pm_planes_host.hip) enqueues from its result and decides nothing itself,
// pm_debug_match_plan (include/pm/testing.h) returns it without a handle or a device, tests/test_match_plan.py pins it and
// tests/test_match_schedule.py counts on the device what every route launches.  No HIP header: this compiles with a host
// compiler alone (tests/cpp/match_plan_main.cpp).  No choice made here changes a result.
#pragma once

#include "pm/patchmatch.h"

namespace pm {

// The A/B knobs of the tuning build (pm_tune.hpp; pm_engine.hip::match_knobs reads them once).  The shipped library runs
// the defaults.
struct MatchKnobs {
  bool view_streams = true;  // PM_VIEW_STREAMS=0: both views on the handle's stream
  // PM_PAIR_CHUNK.  Two pairs advanced through every launch together run at 408 pairs/s where one runs at 373 -- a single
  // pair leaves SIMDs short of wavefronts -- while 4 or 32 in lockstep fall back to 368 / 357 (working sets):
  // profiles/r03_pair_lanes.txt.
  int pair_chunk = 2;
  bool plane_lanes = true;   // PM_PLANES_LANES=1: a plane-mode batch through every launch on one stream
};

enum MatchRoute {
  kRoutePlanes = 0,      // PM_MODE_PLANES: one head for all pairs on the handle's stream, then one or two lanes
  kRouteOneStream = 1,   // head and every view on the handle's stream
  kRouteSharedHead = 2,  // the head once for both views on the handle's stream, then the views on two streams (BGR input)
  kRouteViewHeads = 3,   // each view with its own head on its own stream
  kRouteChunks = 4,      // chunks of pair_chunk pairs one behind the other on the view streams, cross-checks on s_out
};

struct MatchPlan {
  int route = kRouteOneStream;
  int n_views = 1;
  bool self_seed[2] = {false, false};  // view v's seed map is computed on the device (sparse_init and no map given)
  // chunks (kRouteChunks, and the frames of a sequence): pairs per chunk, and whether a chunk's head runs aside on the
  // upload stream -- it does when a view seeds itself (measured, frame sequence at 720p: self-seeded 396 -> 401 pairs/s
  // with the head aside, seeded 410 -> 402: without the seeder the head is too short to pay for one more cross-queue wait)
  int pair_chunk = 2;
  bool head_aside = false;
  int lane_pairs[2] = {0, 0};  // kRoutePlanes: pairs of the lane on the handle's stream / on the second view's stream
  // The rest depends on the parameters alone (callers without a call at hand plan an empty one).
  // frame sequences (pm_submit_*, pm_match_batch_u8): frames run as chunks over the view streams (else as calls on the
  // handle's stream), and a frame may be held for a partner while the device is busy
  bool seq_chunks = false;
  bool seq_hold = false;
  // what must exist before a capture opens (creating events or device memory is not capturable)
  bool need_view_events = false, need_slot_events = false, need_second_seed_scratch = false;
};

// n pairs; seed_l / seed_r: that view's seed maps are given; bgr: the input is BGR (pm_match_bgr_device).
inline MatchPlan plan_match(const pm_params& p, int n, bool seed_l, bool seed_r, bool bgr,
                            const MatchKnobs& k = MatchKnobs()) {
  MatchPlan m;
  const bool planes = p.mode == PM_MODE_PLANES, lr = p.left_right_check != 0;
  m.n_views = lr ? 2 : 1;
  m.self_seed[0] = p.sparse_init && !seed_l;
  m.self_seed[1] = p.sparse_init && !seed_r && lr;
  m.pair_chunk = k.pair_chunk < 1 ? 1 : k.pair_chunk;
  m.head_aside = m.self_seed[0] || m.self_seed[1];
  const bool two_streams = !planes && lr && k.view_streams;
  if (planes) {
    m.route = kRoutePlanes;
    const bool two = k.plane_lanes && n >= 2;  // each lane's launches fill the other's tails (tools/multi_handle.py)
    m.lane_pairs[0] = two ? (n + 1) / 2 : n;
    m.lane_pairs[1] = two ? n / 2 : 0;
  } else if (!two_streams) {
    m.route = kRouteOneStream;
  } else if (bgr) {
    m.route = kRouteSharedHead;
  } else {
    m.route = n > m.pair_chunk ? kRouteChunks : kRouteViewHeads;
  }
  m.seq_chunks = two_streams;
  m.seq_hold = (m.seq_chunks || planes) && m.pair_chunk >= 2;
  m.need_view_events = m.need_slot_events = !planes && lr;
  m.need_second_seed_scratch = p.sparse_init != 0;
  return m;
}

}  // namespace pm
