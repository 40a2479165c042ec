// tiled_steps_main.cpp -- plan_tiled (csrc/pm_tiled_steps.hpp) on a host alone, for a sanitizer run:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iocean-perception_amd/csrc
//       tests/cpp/tiled_steps_main.cpp -o tiled_steps_main && ./tiled_steps_main
// For 1..9 bands, 1..3 iterations, both schedules and every round count 0..n-1 it checks what the exactness of the row-tiled
// mode rests on: rows are taken only after they were published (into that buffer, for that band) and no buffer is
// overwritten before its reader came; the exchange counts; who asks ROW_MOVED; and, by a symbolic run in which a band's
// boundary row is a term over the row its sweep started from, that n - 1 rounds and the pipelined schedule leave every
// band with the sweep that continued from its predecessor's FINAL row -- and that fewer rounds do not, and that ROW_MOVED
// then notices.  Exit status 0 = clean.
#include <cstdio>
#include <map>
#include <utility>
#include <vector>

#include "pm_tiled_steps.hpp"

namespace {

long g_bad = 0;
int g_n, g_it, g_schedule, g_rounds;
void expect(bool ok, const char* what, const pm::TiledStep* s = nullptr) {
  if (ok) return;
  if (g_bad++ >= 20) return;
  std::fprintf(stderr, "%s: %d bands, %d iterations, schedule %d, %d rounds", what, g_n, g_it, g_schedule, g_rounds);
  if (s)
    std::fprintf(stderr, "; step op %d band %d iteration %d pass %d round %d peer %d buffer %d", s->op, s->band, s->iteration,
                 s->pass, s->round, s->peer, s->buffer);
  std::fprintf(stderr, "\n");
}

bool takes(const pm::TiledStep& s) {
  return s.op == PM_TILED_OP_PRESWEEP || s.op == PM_TILED_OP_EXCHANGE_ROUND || s.op == PM_TILED_OP_SET_ROW;
}

// a row as a term: what a sweep of `band` leaves in its boundary row when it started from the row `from`
struct Terms {
  std::map<std::pair<int, int>, int> ids;
  int next = 1;  // 0: no row (the first band of a sweep direction starts from the image border)
  int fresh() { return next++; }
  int swept(int band, int from) {
    auto it = ids.find({band, from});
    return it != ids.end() ? it->second : ids[{band, from}] = next++;
  }
};

void check(int n, int iterations, int schedule, int rounds) {
  g_n = n, g_it = iterations, g_schedule = schedule, g_rounds = rounds;
  const bool pipelined = schedule == PM_TILED_SCHEDULE_PIPELINED;
  const std::vector<pm::TiledStep> steps = pm::plan_tiled(n, iterations, schedule, rounds);
  struct Sent {
    int reader = -1;  // the band the row was published for
    bool written = false, read = true;
    int term = 0;
  };
  std::vector<Sent> sent((size_t)n * 2);
  std::vector<int> row((size_t)n, 0), from((size_t)n, 0), last((size_t)n, -1);
  Terms terms;
  long exchanges = 0, in_pass = 0, moved_in_pass = 0, fired = 0;
  int pass_of = -1, it_of = -1;
  auto pos_of = [&](int band, int pass) { return pass == 1 ? band : n - 1 - band; };
  // a vertical pass is over: counts, and did every band sweep from its predecessor's final row?
  auto close_pass = [&]() {
    if (pass_of != 1 && pass_of != 3) return;
    long want = n - 1;
    for (int r = 0; r < rounds && !pipelined; ++r) want += n - 1 - r;
    expect(in_pass == want, "exchanges of a vertical pass");
    expect(moved_in_pass == (pipelined ? 0 : n - 1), "ROW_MOVED: once per band with a successor");
    bool exact = true;
    int final_row = 0;
    for (int pos = 0; pos < n; ++pos) {
      const int band = pass_of == 1 ? pos : n - 1 - pos;
      final_row = terms.swept(band, final_row);
      exact = exact && row[(size_t)band] == final_row;
    }
    const bool enough = pipelined || rounds >= n - 1;
    expect(exact == enough, enough ? "a band did not sweep from its predecessor's final row" : "too few rounds look exact");
    if (!pipelined) expect((fired > 0) == !enough, enough ? "ROW_MOVED fires on an exact pass" : "ROW_MOVED misses a stale band");
    in_pass = moved_in_pass = fired = 0;
  };
  for (const pm::TiledStep& s : steps) {
    expect(s.band >= 0 && s.band < n && s.iteration >= -1 && s.iteration < iterations, "band or iteration out of range", &s);
    if (s.pass != pass_of || s.iteration != it_of) {
      close_pass();
      pass_of = s.pass, it_of = s.iteration;
      if (s.pass == 1 || s.pass == 3)  // what the rows hold before the pass is anybody's guess
        for (int j = 0; j < n; ++j) row[(size_t)j] = terms.fresh(), from[(size_t)j] = 0;
    }
    const bool vertical = s.pass == 1 || s.pass == 3;
    const size_t b = (size_t)s.band;
    if (takes(s) && s.peer >= 0) {
      expect(vertical && s.peer == s.band + (s.pass == 1 ? -1 : 1) && (s.buffer == 0 || s.buffer == 1), "not the predecessor's row", &s);
      Sent& q = sent[(size_t)s.peer * 2 + (size_t)(s.buffer & 1)];
      expect(q.written && !q.read && q.reader == s.band, "takes a row that was not published for it", &s);
      q.read = true;
      from[b] = q.term;
      ++exchanges, ++in_pass;
      expect(s.copy == (s.op == PM_TILED_OP_PRESWEEP), "only the guess is compared with a later row", &s);
    } else if (takes(s)) {
      expect(s.op == PM_TILED_OP_PRESWEEP && pos_of(s.band, s.pass) == 0, "a band with a predecessor takes no row", &s);
    }
    switch (s.op) {
      case PM_TILED_OP_PUBLISH: {
        expect(vertical && (s.buffer == 0 || s.buffer == 1), "PUBLISH outside a vertical pass", &s);
        const int p = pos_of(s.band, s.pass);
        expect(s.peer == (p + 1 < n ? s.band + (s.pass == 1 ? 1 : -1) : -1), "published for another band than the successor", &s);
        Sent& q = sent[b * 2 + (size_t)(s.buffer & 1)];
        expect(q.read, "PUBLISH overwrites a row its reader has not taken", &s);
        q = Sent{s.peer, true, s.peer < 0, row[b]};
        last[b] = s.buffer;
        break;
      }
      case PM_TILED_OP_SWEEP:
        if (vertical) row[b] = terms.swept(s.band, from[b]);
        break;
      case PM_TILED_OP_EXCHANGE_ROUND:  // the changed columns are re-swept from the snapshot: a sweep from the new row
        expect(!pipelined && s.round >= 0 && s.round < rounds && pos_of(s.band, s.pass) > s.round, "EXCHANGE_ROUND of a final band", &s);
        row[b] = terms.swept(s.band, from[b]);
        break;
      case PM_TILED_OP_ROW_MOVED:
        expect(!pipelined && vertical && pos_of(s.band, s.pass) + 1 < n, "ROW_MOVED of a band without a successor", &s);
        expect(s.buffer == last[b], "ROW_MOVED against another row than the last published", &s);
        ++moved_in_pass;
        if (row[b] != sent[b * 2 + (size_t)(s.buffer & 1)].term) ++fired;
        break;
      case PM_TILED_OP_PRESWEEP:
        expect(!pipelined && vertical, "PRESWEEP in the pipelined schedule", &s);
        break;
      case PM_TILED_OP_SET_ROW:
        expect(pipelined && vertical, "SET_ROW in the speculative schedule", &s);
        break;
      default:
        expect(s.op >= PM_TILED_OP_BEGIN && s.op <= PM_TILED_OP_SET_ROW && s.peer == -1 && s.buffer == -1, "unknown step", &s);
    }
  }
  close_pass();
  for (const Sent& q : sent) expect(q.read, "a published row is never taken");
  if (pipelined) expect(exchanges == 2L * iterations * (n - 1), "exchanges of the pipelined schedule");
  long per_band[3] = {0, 0, 0};  // BEGIN, BACKGROUND, FINISH
  for (const pm::TiledStep& s : steps)
    per_band[0] += s.op == PM_TILED_OP_BEGIN, per_band[1] += s.op == PM_TILED_OP_BACKGROUND, per_band[2] += s.op == PM_TILED_OP_FINISH;
  expect(per_band[0] == n && per_band[1] == n && per_band[2] == n, "BEGIN, BACKGROUND, FINISH once per band");
}

}  // namespace

int main() {
  long n_plans = 0;
  for (int n = 1; n <= 9; ++n)
    for (int iterations = 1; iterations <= 3; ++iterations)
      for (int schedule : {PM_TILED_SCHEDULE_SPECULATIVE, PM_TILED_SCHEDULE_PIPELINED})
        for (int rounds = 0; rounds <= n - 1; ++rounds) {
          check(n, iterations, schedule, rounds);
          ++n_plans;
        }
  // a negative or too large round count is the exact one
  for (int n = 1; n <= 9; ++n)
    for (int rounds : {-1, n, 1 << 20}) {
      const std::vector<pm::TiledStep> a = pm::plan_tiled(n, 2, PM_TILED_SCHEDULE_SPECULATIVE, rounds),
                                       b = pm::plan_tiled(n, 2, PM_TILED_SCHEDULE_SPECULATIVE, n - 1);
      g_n = n, g_rounds = rounds;
      expect(a.size() == b.size() && pm::tiled_rounds(n, rounds) == n - 1, "round count not clamped to n - 1");
    }
  // the image rows of a band's boundaries
  pm_tile t{100, 17, 20, 30};
  const pm::BoundaryRows down = pm::boundary_rows(t, 1), up = pm::boundary_rows(t, 3);
  expect(down.out == 49 && down.pred == 19 && up.out == 20 && up.pred == 50, "boundary_rows");
  std::printf("plan_tiled: %ld plans, %ld broken\n", n_plans, g_bad);
  return g_bad ? 1 : 0;
}
