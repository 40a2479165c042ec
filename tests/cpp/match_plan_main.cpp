// match_plan_main.cpp -- plan_match (csrc/pm_match_plan.hpp) on a host alone, for a sanitizer run:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iocean-perception_amd/csrc
//       tests/cpp/match_plan_main.cpp -o match_plan_main && ./match_plan_main
// Walks modes, view counts, batch sizes, seed maps, input kinds and knobs, and checks what every consumer of the plan
// relies on: one route per call, lanes and chunks that cover the batch, self-seeding only where the seeder is on and the
// view exists, a head aside only where a view seeds itself.  Exit status 0 = clean.
#include <cstdio>
#include <cstring>

#include "pm_match_plan.hpp"

namespace {

long g_bad = 0;
void expect(bool ok, const char* what, const pm::MatchPlan& m, int n) {
  if (ok) return;
  if (g_bad++ < 20)
    std::fprintf(stderr, "%s: n %d route %d views %d self-seed %d %d chunk %d aside %d lanes %d + %d seq %d %d\n", what, n,
                 m.route, m.n_views, m.self_seed[0], m.self_seed[1], m.pair_chunk, m.head_aside, m.lane_pairs[0],
                 m.lane_pairs[1], m.seq_chunks, m.seq_hold);
}

void check(const pm_params& p, int n, bool sl, bool sr, bool bgr, const pm::MatchKnobs& k) {
  const pm::MatchPlan m = pm::plan_match(p, n, sl, sr, bgr, k);
  const bool planes = p.mode == PM_MODE_PLANES, lr = p.left_right_check != 0;
  expect(m.n_views == (lr ? 2 : 1), "views", m, n);
  expect(m.pair_chunk >= 1, "pairs per chunk", m, n);
  expect((m.route == pm::kRoutePlanes) == planes, "plane mode has its own route", m, n);
  expect(m.self_seed[0] == (p.sparse_init && !sl) && m.self_seed[1] == (p.sparse_init && !sr && lr), "self-seeding", m, n);
  expect(m.head_aside == (m.self_seed[0] || m.self_seed[1]), "a head aside without a seeder (or the reverse)", m, n);
  if (planes) {
    expect(m.lane_pairs[0] + m.lane_pairs[1] == n && m.lane_pairs[0] >= m.lane_pairs[1] &&
               m.lane_pairs[0] - m.lane_pairs[1] <= (m.lane_pairs[1] ? 1 : n),
           "lanes do not cover the batch", m, n);
    expect(!m.seq_chunks, "plane-mode frames do not run over the view streams", m, n);
  } else {
    expect(m.lane_pairs[0] == 0 && m.lane_pairs[1] == 0, "lanes outside plane mode", m, n);
    const bool two = lr && k.view_streams;
    expect((m.route == pm::kRouteOneStream) == !two, "one stream exactly without two view streams", m, n);
    if (two) expect(m.route == (bgr ? pm::kRouteSharedHead : n > m.pair_chunk ? pm::kRouteChunks : pm::kRouteViewHeads), "route", m, n);
    expect(m.seq_chunks == two, "sequences run as chunks exactly where single calls use two streams", m, n);
  }
  expect(!m.seq_hold || m.pair_chunk >= 2, "a held frame needs room for a partner in its chunk", m, n);
  expect(m.need_view_events == m.need_slot_events && m.need_second_seed_scratch == (p.sparse_init != 0), "capture needs", m, n);
}

}  // namespace

int main() {
  long n_plans = 0;
  const int batches[] = {1, 2, 3, 4, 5, 31, 32, 1000};
  const int chunks[] = {-1, 0, 1, 2, 3, 4, 64};
  for (int mode = PM_MODE_SCALAR; mode <= PM_MODE_PLANES; ++mode)
    for (int lr = 0; lr < 2; ++lr)
      for (int sparse = 0; sparse < 2; ++sparse)
        for (int n : batches)
          for (int bits = 0; bits < 8; ++bits)
            for (int vs = 0; vs < 2; ++vs)
              for (int lanes = 0; lanes < 2; ++lanes)
                for (int chunk : chunks) {
                  pm_params p;
                  std::memset(&p, 0, sizeof(p));
                  p.mode = mode;
                  p.left_right_check = lr;
                  p.sparse_init = sparse;
                  pm::MatchKnobs k;
                  k.view_streams = vs != 0;
                  k.plane_lanes = lanes != 0;
                  k.pair_chunk = chunk;
                  check(p, n, (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, k);
                  ++n_plans;
                }
  std::printf("plan_match: %ld plans, %ld broken\n", n_plans, g_bad);
  return g_bad ? 1 : 0;
}
