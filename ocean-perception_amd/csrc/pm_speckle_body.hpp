// pm_speckle_body.hpp -- the per-thread code of pm_filter_speckles (include/pm/imaging.h): the runs of a tile row from a
// 64-bit mask, union and find, and the items of the merge, flatten and apply launches.  No HIP in it and no kernel: every
// access to memory that another thread may write at the same time goes through a small policy type `Mem`
//   int  load(const int* p)        a read that may run beside writers        void store(int* p, int v)
//   int  atomic_min(int* p, int v) returns what *p held                      void atomic_add(int* p, int v)
// so that the kernels (pm_speckle.hpp: LDS and global-memory policies) and a plain g++ build (tests/cpp/
// speckle_host_main.cpp, under the sanitizers: SpeckleSerialMem below) share ONE statement of it.  The definition it is held
// to BIT FOR BIT is tests/speckle_ref.py.
//
// The forest.  labels[p] is the parent of pixel p (a linear index), p itself at a root, -1 at an invalid pixel.  INVARIANT:
// every value ever stored in labels[p] is <= p, and a link is only ever made between two pixels of one component.  So
// every walk towards a root strictly decreases and ends, a root is the smallest index of its tree, and once every edge has
// been united the root is the component's smallest index: the canonical label, whatever the schedule was.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PM_SPECKLE_HD __host__ __device__ __forceinline__
#else
#define PM_SPECKLE_HD inline
#endif

namespace pm {

constexpr int kSpeckleTileCols = 64;  // pixels of a workgroup's tile along a row: one wavefront per tile row
constexpr int kSpeckleTileRows = 16;  // ... and its rows
constexpr int kSpeckleTileCells = kSpeckleTileCols * kSpeckleTileRows;

// valid iff d > 0: 0, -0.0, negatives and NaN are not, +inf is
PM_SPECKLE_HD bool speckle_valid(float d) { return d > 0.f; }

// the edge rule, in binary64; a NaN difference (inf - inf) never joins, an infinite one neither (max_diff is finite)
PM_SPECKLE_HD bool speckle_joined(float a, float b, float max_diff) {
  return a > 0.f && b > 0.f && __builtin_fabs((double)a - (double)b) <= (double)max_diff;
}

// ---- the runs of one tile row.  `starts`: bit k set iff lane k is NOT joined to lane k - 1 (bit 0 is always set; an
// invalid lane is joined to nothing and so starts a run of its own).
// The first lane of `lane`'s run: the highest set bit at or below it.
PM_SPECKLE_HD int speckle_run_start(uint64_t starts, int lane) {
  return 63 - __builtin_clzll((starts | 1ull) & (~0ull >> (63 - lane)));
}
// The lanes of the run that begins at `lane` (a set bit of starts): up to the next set bit, or the row's end.
PM_SPECKLE_HD int speckle_run_length(uint64_t starts, int lane) {
  const uint64_t above = lane == 63 ? 0ull : starts >> (lane + 1);
  return above ? __builtin_ctzll(above) + 1 : 64 - lane;
}
// Which lanes unite with the row above.  `up`: bit k set iff lane k is joined to lane k of the row above.  Lane k may leave
// it to lane k - 1 where k - 1 is joined upwards too and lies in the same run as k in BOTH rows: that union is this one.
PM_SPECKLE_HD uint64_t speckle_link_mask(uint64_t up, uint64_t starts, uint64_t starts_above) {
  return up & ~((up << 1) & ~starts & ~starts_above);
}

// ---- union-find ----------------------------------------------------------------------------------------------------------
// The root above x.  Terminates: by the invariant every parent read is < x until it equals x (a value read late or stale was
// once stored in that entry and obeys the invariant too), so x strictly decreases and is >= 0.
template <class Mem>
PM_SPECKLE_HD int speckle_find(const Mem& m, const int* labels, int x) {
  for (int p = m.load(labels + x); p != x; p = m.load(labels + x)) x = p;
  return x;
}

// Unites the trees of a and b.  Only what atomic_min RETURNS decides: it is asked to hang the larger index a below the
// smaller b; where a was a root (it returns a) the link is made and the work is done; otherwise a hung below `old` already,
// the minimum has kept the smaller parent, and what is left is to unite old with b.  Terminates: old < a, so max(a, b)
// strictly decreases with every turn and is >= 0.  It waits for no other thread.
template <class Mem>
PM_SPECKLE_HD void speckle_union(const Mem& m, int* labels, int a, int b) {
  a = speckle_find(m, labels, a);  // a shortcut only: any member of the tree would do
  b = speckle_find(m, labels, b);
  while (a != b) {
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = m.atomic_min(labels + a, b);
    if (old == a) break;
    a = old;
  }
}

// ---- launch 1: one tile in a workgroup's LDS.  `lab` and `cnt` have kSpeckleTileCells entries, cell = row * 64 + lane.
PM_SPECKLE_HD int speckle_tile_init(int row, int lane, bool valid, uint64_t starts) {
  return valid ? row * kSpeckleTileCols + speckle_run_start(starts, lane) : -1;
}
// lane `lane` of tile row `row` >= 1, a set bit of speckle_link_mask: its run and the one above it become one tree
template <class Mem>
PM_SPECKLE_HD void speckle_tile_link(const Mem& m, int* lab, int row, int lane) {
  speckle_union(m, lab, row * kSpeckleTileCols + lane, (row - 1) * kSpeckleTileCols + lane);
}
// After every link of the tile: the cell's root, stored into its own entry (other threads may be walking through it: they
// read the old parent or the root, both above them in the tree).  The first lane of a run adds the run's length to the
// root's count, so a tile makes one add per run, not one per pixel.  -1 for an invalid cell.
template <class Mem>
PM_SPECKLE_HD int speckle_tile_flatten(const Mem& m, int* lab, int* cnt, int row, int lane, bool valid, uint64_t starts) {
  if (!valid) return -1;
  const int cell = row * kSpeckleTileCols + lane;
  const int root = speckle_find(m, lab, cell);
  if (root != cell) m.store(lab + cell, root);
  if ((starts >> lane) & 1) m.atomic_add(cnt + root, speckle_run_length(starts, lane));
  return root;
}

struct SpeckleArgs {
  const float* disp;
  int rows, cols;
  float max_diff;
  int* labels;  // [rows][cols] working labels: the forest
  int* sizes;   // [rows][cols] pixel counts, meaningful at roots
};

// The tile's results for pixel (x, y) inside the image: the working label is the image index of the tile-local root (cells
// and image indices are both row-major, so the smaller cell is the smaller index), the count sits at the root alone.
PM_SPECKLE_HD void speckle_tile_store(const SpeckleArgs& a, int x0, int y0, int row, int lane, int root, const int* cnt) {
  const size_t p = (size_t)(y0 + row) * a.cols + (x0 + lane);
  const int cell = row * kSpeckleTileCols + lane;
  a.labels[p] = root < 0 ? -1 : (y0 + root / kSpeckleTileCols) * a.cols + x0 + root % kSpeckleTileCols;
  a.sizes[p] = root == cell ? cnt[cell] : 0;
}

// ---- launch 2: the edges that cross a tile border.  Items 0 .. speckle_merge_items - 1: first the pixels of every tile's
// first column but the image's (their neighbour to the left lies in the next tile), then those of every first row.
PM_SPECKLE_HD int speckle_tiles_x(int cols) { return (cols + kSpeckleTileCols - 1) / kSpeckleTileCols; }
PM_SPECKLE_HD int speckle_tiles_y(int rows) { return (rows + kSpeckleTileRows - 1) / kSpeckleTileRows; }
PM_SPECKLE_HD long long speckle_merge_items(int rows, int cols) {
  return (long long)(speckle_tiles_x(cols) - 1) * rows + (long long)(speckle_tiles_y(rows) - 1) * cols;
}

template <class Mem>
PM_SPECKLE_HD void speckle_merge_item(const Mem& m, const SpeckleArgs& a, long long item) {
  const long long vertical = (long long)(speckle_tiles_x(a.cols) - 1) * a.rows;
  int x, y, dx, dy;  // (dx, dy): the step to the neighbour across the border; the border itself runs along (dy, dx)
  if (item < vertical) {
    y = (int)(item % a.rows), x = ((int)(item / a.rows) + 1) * kSpeckleTileCols, dx = 1, dy = 0;
  } else {
    const long long k = item - vertical;
    x = (int)(k % a.cols), y = ((int)(k / a.cols) + 1) * kSpeckleTileRows, dx = 0, dy = 1;
  }
  const int p = y * a.cols + x, q = (y - dy) * a.cols + (x - dx);
  if (!speckle_joined(a.disp[p], a.disp[q], a.max_diff)) return;
  if (dx ? y > 0 : x > 0) {
    // The border pixel before this one, pp, and its neighbour qq.  Where they are joined, their item unites them (or leaves
    // it to the one before, and so on back to one that does).  If p has been seen with the parent pp has been seen with,
    // and q with qq's, p sits in pp's tree and q in qq's for good, and that union is this one.
    const int pp = (y - dx) * a.cols + (x - dy), qq = (y - dx - dy) * a.cols + (x - dy - dx);
    if (speckle_joined(a.disp[pp], a.disp[qq], a.max_diff) && m.load(a.labels + p) == m.load(a.labels + pp) &&
        m.load(a.labels + q) == m.load(a.labels + qq))
      return;
  }
  speckle_union(m, a.labels, p, q);
}

// ---- launch 3: every pixel takes its root; every tile-local root that is not the root hands its count over.
// Storing the root while other threads walk through this entry is benign: they read the old parent or the root, and both
// are above them in the tree (no link is made in this launch).  The adds are integer adds to the root's entry, which
// nobody reads here for its value: one per tile-local component, in any order.
template <class Mem>
PM_SPECKLE_HD void speckle_flatten_item(const Mem& m, const SpeckleArgs& a, int p) {
  const int parent = m.load(a.labels + p);
  if (parent < 0) return;
  const int root = speckle_find(m, a.labels, parent);
  if (root != parent) m.store(a.labels + p, root);
  if (root == p) return;
  const int count = a.sizes[p];  // written by launch 1; adds go to roots only, and p is none
  if (count > 0) m.atomic_add(a.sizes + root, count);
}

// ---- launch 4: the outputs of pixel p; a null output is not written.  Returns whether the pixel was removed.
struct SpeckleOut {
  float* out;       // may be a.disp
  int32_t* labels;
  int32_t* sizes;
  int max_size;
};
PM_SPECKLE_HD bool speckle_apply_item(const SpeckleArgs& a, const SpeckleOut& o, int p) {
  const int label = a.labels[p];
  const int size = label < 0 ? 0 : a.sizes[label];
  const bool removed = label >= 0 && size <= o.max_size;
  if (o.out) {
    const float d = a.disp[p];  // read before the store: out may be disp
    o.out[p] = removed ? 0.f : d;
  }
  if (o.labels) o.labels[p] = label;
  if (o.sizes) o.sizes[p] = size;
  return removed;
}

// The policy of one thread at a time (host builds; tests/cpp/speckle_host_main.cpp).
struct SpeckleSerialMem {
  int load(const int* p) const { return *p; }
  void store(int* p, int v) const { *p = v; }
  int atomic_min(int* p, int v) const {
    const int old = *p;
    if (v < old) *p = v;
    return old;
  }
  void atomic_add(int* p, int v) const { *p += v; }
};

}  // namespace pm
