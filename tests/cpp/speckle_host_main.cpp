// speckle_host_main.cpp -- runs pm_filter_speckles' own per-thread code (csrc/pm_speckle_body.hpp: the row runs from a
// 64-bit mask, union, find, the merge, flatten and apply items -- what the threads of the four kernels run) on the HOST with
// plain g++ and -fsanitize=address,undefined; it needs no library and no GPU.  A map is labelled tile by tile as the launch
// grid walks it; every tile is three heap allocations of EXACTLY a workgroup's LDS arrays and the scratch and every output
// are allocations of exactly their bytes, so an index outside any of them is reported.  The items of every launch -- the
// links of a tile, the merge items, the flatten items -- then run one at a time in forward, reverse and shuffled order, and
// labels, sizes, output and the removed count must equal a flood fill written below, every time.
// This covers indexing and SEQUENTIAL order-independence.  It does not cover concurrent interleavings: those rest on the
// argument next to speckle_union (only what the atomics return decides) and on the GPU tests.
//   speckle_host_main            exit status 0: every case equal; 1: a mismatch (named on stderr)
//   speckle_host_main --corrupt  flips one expected label first: must exit 1 (the program does compare)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>
#include <vector>

#include "pm_speckle_body.hpp"

using namespace pm;

static uint32_t g_rng = 12345u;
static uint32_t rnd() { return g_rng = g_rng * 1664525u + 1013904223u; }
static float uniform() { return (float)(rnd() >> 8) / 16777216.f; }

static std::vector<long long> order_of(long long n, int order) {
  std::vector<long long> v((size_t)n);
  std::iota(v.begin(), v.end(), 0LL);
  if (order == 1)
    for (long long i = 0; i < n / 2; ++i) std::swap(v[(size_t)i], v[(size_t)(n - 1 - i)]);
  if (order == 2)
    for (long long i = n - 1; i > 0; --i) std::swap(v[(size_t)i], v[(size_t)(rnd() % (uint32_t)(i + 1))]);
  return v;
}

// k_speckle_local for the tile at (x0, y0), thread by thread; the barriers are the ends of the loops
static void run_tile(const SpeckleArgs& a, int x0, int y0, int order) {
  const SpeckleSerialMem mem;
  std::unique_ptr<float[]> tile(new float[kSpeckleTileCells]);
  std::unique_ptr<int[]> lab(new int[kSpeckleTileCells]), cnt(new int[kSpeckleTileCells]), root(new int[kSpeckleTileCells]);
  uint64_t starts[kSpeckleTileRows], up[kSpeckleTileRows];
  for (int cell = 0; cell < kSpeckleTileCells; ++cell) {
    const int x = x0 + cell % kSpeckleTileCols, y = y0 + cell / kSpeckleTileCols;
    tile[cell] = x < a.cols && y < a.rows ? a.disp[(size_t)y * a.cols + x] : 0.f;
    cnt[cell] = 0;
  }
  for (int row = 0; row < kSpeckleTileRows; ++row) {
    starts[row] = up[row] = 0;
    for (int lane = 0; lane < kSpeckleTileCols; ++lane) {  // the two ballots of the row's wavefront
      const int cell = row * kSpeckleTileCols + lane;
      const bool joined_left = lane > 0 && speckle_joined(tile[cell], tile[cell - 1], a.max_diff);
      const bool joined_up = row > 0 && speckle_joined(tile[cell], tile[cell - kSpeckleTileCols], a.max_diff);
      starts[row] |= (uint64_t)!joined_left << lane;
      up[row] |= (uint64_t)joined_up << lane;
    }
    for (int lane = 0; lane < kSpeckleTileCols; ++lane)
      lab[row * kSpeckleTileCols + lane] = speckle_tile_init(row, lane, speckle_valid(tile[row * kSpeckleTileCols + lane]), starts[row]);
  }
  for (long long cell : order_of(kSpeckleTileCells, order)) {
    const int row = (int)cell / kSpeckleTileCols, lane = (int)cell % kSpeckleTileCols;
    if (row > 0 && ((speckle_link_mask(up[row], starts[row], starts[row - 1]) >> lane) & 1)) speckle_tile_link(mem, lab.get(), row, lane);
  }
  for (long long cell : order_of(kSpeckleTileCells, order)) {
    const int row = (int)cell / kSpeckleTileCols, lane = (int)cell % kSpeckleTileCols;
    root[cell] = speckle_tile_flatten(mem, lab.get(), cnt.get(), row, lane, speckle_valid(tile[cell]), starts[row]);
  }
  for (int cell = 0; cell < kSpeckleTileCells; ++cell) {
    const int row = cell / kSpeckleTileCols, lane = cell % kSpeckleTileCols;
    if (x0 + lane < a.cols && y0 + row < a.rows) speckle_tile_store(a, x0, y0, row, lane, root[cell], cnt.get());
  }
}

struct Result {
  std::vector<float> out;
  std::vector<int32_t> labels, sizes;
  int removed = 0;
};

// the four launches of pm_filter_speckles, one item at a time
static Result run_body(const std::vector<float>& disp, int rows, int cols, float max_diff, int max_size, int order, bool inplace) {
  const int pixels = rows * cols;
  const SpeckleSerialMem mem;
  std::unique_ptr<float[]> map(new float[pixels]);
  memcpy(map.get(), disp.data(), sizeof(float) * pixels);
  std::unique_ptr<int[]> labels(new int[pixels]), sizes(new int[pixels]);
  const SpeckleArgs a = {map.get(), rows, cols, max_diff, labels.get(), sizes.get()};
  const int tiles_x = speckle_tiles_x(cols);
  for (long long t : order_of((long long)tiles_x * speckle_tiles_y(rows), order))
    run_tile(a, (int)(t % tiles_x) * kSpeckleTileCols, (int)(t / tiles_x) * kSpeckleTileRows, order);
  for (long long item : order_of(speckle_merge_items(rows, cols), order)) speckle_merge_item(mem, a, item);
  for (long long p : order_of(pixels, order)) speckle_flatten_item(mem, a, (int)p);
  Result r;
  r.labels.resize(pixels), r.sizes.resize(pixels);
  std::unique_ptr<float[]> out(new float[pixels]);
  const SpeckleOut o = {inplace ? map.get() : out.get(), r.labels.data(), r.sizes.data(), max_size};
  for (long long p : order_of(pixels, order)) r.removed += speckle_apply_item(a, o, (int)p) ? 1 : 0;
  r.out.assign(o.out, o.out + pixels);
  return r;
}

// the definition, as a flood fill in row-major order: the first pixel met of a component is its smallest index
static Result run_fill(const std::vector<float>& disp, int rows, int cols, float max_diff, int max_size) {
  const int pixels = rows * cols;
  Result r;
  r.out = disp;
  r.labels.assign(pixels, -1), r.sizes.assign(pixels, 0);
  auto joined = [&](int p, int q) {
    const float dp = disp[p], dq = disp[q];
    return dp > 0.f && dq > 0.f && std::fabs((double)dp - (double)dq) <= (double)max_diff;
  };
  std::vector<int> members;
  for (int s = 0; s < pixels; ++s) {
    if (!(disp[s] > 0.f) || r.labels[s] >= 0) continue;
    members.assign(1, s);
    r.labels[s] = s;
    for (size_t k = 0; k < members.size(); ++k) {
      const int p = members[k], y = p / cols, x = p % cols;
      const int near[4] = {x + 1 < cols ? p + 1 : -1, x > 0 ? p - 1 : -1, y + 1 < rows ? p + cols : -1, y > 0 ? p - cols : -1};
      for (int q : near)
        if (q >= 0 && r.labels[q] < 0 && joined(p, q)) r.labels[q] = s, members.push_back(q);
    }
    for (int p : members) {
      r.sizes[p] = (int)members.size();
      if ((int)members.size() <= max_size) r.out[p] = 0.f, ++r.removed;
    }
  }
  return r;
}

static std::vector<float> make_map(int kind, int rows, int cols) {
  static const float specials[] = {0.f, -0.f, -1.f, -37.5f, std::numeric_limits<float>::quiet_NaN(),
                                   std::numeric_limits<float>::infinity(), 1e-45f, 1e-39f, 1.1754942e-38f};
  std::vector<float> d((size_t)rows * cols, 0.f);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) {
      float& v = d[(size_t)y * cols + x];
      switch (kind) {
        case 0: v = 10.f; break;                                                                      // constant
        case 1: v = y % 2 == 0 || x == (y % 4 == 1 ? cols - 1 : 0) ? 10.f : 0.f; break;               // serpentine
        case 2: v = x % 2 == 0 || y == rows - 1 ? 10.f : 0.f; break;                                  // comb
        case 3: v = (x + y) % 2 == 0 ? 10.f : 0.f; break;                                             // checkerboard
        case 4: v = y == 0 ? 10.f : y == rows - 1 ? 20.f : x % 2 == 0 ? 10.f : 20.f; break;           // two combs
        case 5: v = uniform() < 0.6f ? 20.f + (float)(int)(uniform() * 6.f) : 0.f; break;             // blobs of 6 levels
        case 6: v = uniform() < 0.95f ? 30.f + 0.25f * (float)(x / 3 + y / 2) : 0.f; break;           // a ramp in steps
        default: v = uniform() < 0.15f ? specials[rnd() % 9u] : uniform() < 0.8f ? 5.f + 2.f * uniform() : 0.f; break;
      }
    }
  return d;
}

int main(int argc, char** argv) {
  const bool corrupt = argc > 1 && !strcmp(argv[1], "--corrupt");
  const int shapes[][2] = {{1, 1}, {1, kSpeckleTileCols + 1}, {kSpeckleTileRows + 1, 1}, {kSpeckleTileRows, kSpeckleTileCols},
                           {kSpeckleTileRows + 1, kSpeckleTileCols + 1}, {2 * kSpeckleTileRows + 3, 2 * kSpeckleTileCols + 5},
                           {37, 53}, {5, 200}};
  int cases = 0, bad = 0;
  for (const auto& s : shapes)
    for (int kind = 0; kind < 8; ++kind) {
      const int rows = s[0], cols = s[1], pixels = rows * cols;
      const std::vector<float> disp = make_map(kind, rows, cols);
      const float max_diff = kind == 4 ? 9.5f : kind == 6 ? 0.25f : 1.f;
      const int max_size = kind == 3 ? 1 : cases % 5 == 0 ? 0 : 20;
      Result want = run_fill(disp, rows, cols, max_diff, max_size);
      if (corrupt && cases == 0) want.labels[0] ^= 1;
      for (int order = 0; order < 3; ++order) {
        const Result got = run_body(disp, rows, cols, max_diff, max_size, order, order == 1);
        const char* what = memcmp(got.labels.data(), want.labels.data(), 4 * (size_t)pixels) ? "labels"
                           : memcmp(got.sizes.data(), want.sizes.data(), 4 * (size_t)pixels) ? "sizes"
                           : memcmp(got.out.data(), want.out.data(), 4 * (size_t)pixels)     ? "out"
                           : got.removed != want.removed                                      ? "removed"
                                                                                              : nullptr;
        if (what) {
          fprintf(stderr, "%s differs from the flood fill: %dx%d, map %d, order %d\n", what, rows, cols, kind, order);
          ++bad;
        }
      }
      ++cases;
    }
  printf("speckle_host_main: %d maps x 3 orders, %d mismatches\n", cases, bad);
  return bad ? 1 : 0;
}
