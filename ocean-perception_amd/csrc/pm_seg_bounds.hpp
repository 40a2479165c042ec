// pm_seg_bounds.hpp -- where k_runblk3 (pm_run3.hpp) cuts a chain into its segments: ONE pure function,
// segment_bounds.  No HIP header: host and device code compile it (tests/cpp/segment_bounds_main.cpp walks it with a host
// compiler alone, pm_debug_segment_bounds exports it).  The kernel computes the same boundaries cooperatively
// (run3_bounds) and tests/test_sweep_segments.py compares the two.  No choice made here changes a result: the fix-up
// rounds end at the sequential sweep whatever the segmentation is.
//
// A segment costs about (its length / nd) + (its stops) run steps, nd = positions a step covers, a stop = a position
// that will not take its predecessor's value.  With a PREDICTION of the stops the boundaries are placed at equal
// cumulative weight, a predicted stop weighing nd and any other position 1, so that the segments of a chain end together
// instead of the one that holds an occlusion ending last.  The prediction is a hint: any flags give valid boundaries.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PM_SEG_HD __host__ __device__
#else
#define PM_SEG_HD
#endif

namespace pm {

constexpr int kMinSegLen = 8;          // positions per segment at least (plan_sweep's seg_len has the same floor)
constexpr int kSegHintMaxSeg = 32;     // hinted boundaries for at most this many segments: one lane each in the kernel
constexpr int kSegHintMaxLen = 4095;   // ... and chains of at most this many positions: 64 blocks of 64, one lane each

// static LDS of k_runblk3's row +1 variants: the staged stop masks, one 64-bit word per 64 positions (pm_sweep_plan.hpp)
constexpr unsigned long kRun3StaticLds = 8ul * ((kSegHintMaxLen + 64) / 64);

// A launch takes a hint only where its chains are long enough to pay for it.  The pre-pass and its barrier sit on every
// chain's path, about three run steps' worth; what balance wins grows with the steps of a chain.  Measured: chains of 1270
// positions gain (1280 x 720), chains of 366 positions lose 4.5 % per call (376 x 240).  The floor is the
// length below which plan_sweep calls a chain short (kShortChain, pm_sweep_plan.hpp).
constexpr int kSegHintMinChain = 400;
PM_SEG_HD inline bool seg_hint_pays(int chain_len) { return chain_len >= kSegHintMinChain; }

// Where the hint of a launch comes from (k_runblk3's `hint` argument, pm_debug_propagate_hinted's hint_modes).
enum SegHint {
  kSegHintNone = 0,   // the equal split
  kSegHintRuns = 1,   // run boundaries of the state the sweep starts from: position j stops iff old[j] != old[j - 1]
  kSegHintPlane = 2,  // the stop-bit plane the same sweep of the previous iteration wrote (PlaneSet::stops)
};

// The equal split: segment s starts at min(n, s * seg_len), seg_len = max(ceil(n / nseg), min_len); a segment that
// starts at n is empty and idles.
PM_SEG_HD inline int equal_seg_len(int n, int nseg, int min_len) {
  const int sl = (n + nseg - 1) / nseg;
  return sl < min_len ? min_len : sl;
}

// true: (flags, n, nseg) take weighted boundaries; false: the equal split
PM_SEG_HD inline bool seg_hint_applies(int n, int nseg, int min_len) {
  return nseg >= 1 && nseg <= kSegHintMaxSeg && n <= kSegHintMaxLen && n >= nseg * min_len;
}

// b[0 .. nseg]: segment s holds the chain positions b[s] .. b[s + 1] - 1.  flags: null, or one byte per position
// (non-zero = predicted stop); n >= 1 positions, nseg >= 1 segments, nd >= 1, min_len >= 1.
//   b[0] = 0, b[nseg] = n, always.
//   Equal split (above) when flags is null, when no flag is set, and when seg_hint_applies() is false.
//   Otherwise w[p] = flags[p] ? nd : 1, W = sum w, and b[s] = the smallest j with w[0] + .. + w[j - 1] >= ceil(s * W / nseg),
//   then pushed up to b[s - 1] + min_len from the left and down to n - (nseg - s) * min_len from the right: strictly
//   increasing, every segment at least min_len long.
PM_SEG_HD inline void segment_bounds(const uint8_t* flags, int n, int nseg, int nd, int min_len, int* b) {
  long long W = 0;
  bool any = false;
  if (flags && seg_hint_applies(n, nseg, min_len))
    for (int p = 0; p < n; ++p) {
      any = any || flags[p] != 0;
      W += flags[p] ? nd : 1;
    }
  if (!any) {
    const int sl = equal_seg_len(n, nseg, min_len);
    for (int s = 0; s <= nseg; ++s) {
      const long long i = (long long)s * sl;
      b[s] = i < n ? (int)i : n;
    }
    b[nseg] = n;
    return;
  }
  b[0] = 0;
  long long P = 0;  // w[0] + .. + w[j - 1]
  int j = 0;
  for (int s = 1; s < nseg; ++s) {
    const long long T = ((long long)s * W + nseg - 1) / nseg;
    while (P < T) {  // T <= W: ends with j <= n
      P += flags[j] ? nd : 1;
      ++j;
    }
    const int lo = b[s - 1] + min_len;
    b[s] = j > lo ? j : lo;
  }
  b[nseg] = n;
  for (int s = nseg - 1; s >= 1; --s) {
    const int hi = n - (nseg - s) * min_len;
    if (b[s] > hi) b[s] = hi;
  }
}

}  // namespace pm
