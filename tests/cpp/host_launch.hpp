// host_launch.hpp -- the launch walk that the programs which run kernel code on the host (tests/cpp/*_host_main.cpp) share:
// every block of a grid and every thread of a block, in launch order or in exactly the reverse, and the per-block sums of the
// flags a thread returns.  The extents come from the code under test (the k*Block* constants and span_blocks() of the
// csrc/*_body.hpp headers); nothing here knows a launch shape.  No HIP in it: a program built by plain g++ may include it.
#pragma once

// i-th of n, counted from the front or from the back
static inline long long nth(long long i, long long n, bool backwards) { return backwards ? n - 1 - i : i; }

// every block of a (gx, gy, gz) grid, x fastest, forwards or backwards: body(block x, block y, block z)
template <typename Body>
static void for_blocks(long long gx, long long gy, long long gz, bool backwards, Body body) {
  for (long long b = 0; b < gx * gy * gz; ++b) {
    const long long at = nth(b, gx * gy * gz, backwards);
    body((int)(at % gx), (int)(at / gx % gy), (int)(at / (gx * gy)));
  }
}

// every thread of a (bx, by) block, x fastest, forwards or backwards: body(thread x, thread y)
template <typename Body>
static void for_threads(int bx, int by, bool backwards, Body body) {
  for (int i = 0; i < bx * by; ++i) {
    const int at = (int)nth(i, bx * by, backwards);
    body(at % bx, at / bx);
  }
}

// A thread's packed flags into its block's sums: counter c owns bits PIXELS * c .. PIXELS * c + PIXELS - 1, one per pixel of
// the thread (the layout of consistency_lane, fuse_lane and tsdf_integrate_lane, whose kernels ballot bit PIXELS * c + k).
template <int PIXELS, int COUNTERS>
static void add_flags(unsigned flags, int (&sums)[COUNTERS]) {
  for (int c = 0; c < COUNTERS; ++c) sums[c] += __builtin_popcount((flags >> (PIXELS * c)) & ((1u << PIXELS) - 1u));
}

// The end of a block: one add(counts + c, sums[c]) per counter that is not zero (add: pm::reproject_add)
template <int COUNTERS, typename Add>
static void flush_sums(int* counts, const int (&sums)[COUNTERS], Add add) {
  for (int c = 0; c < COUNTERS; ++c)
    if (sums[c]) add(counts + c, sums[c]);
}
