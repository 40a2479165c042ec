// pm_cloud.hpp -- the kernels of pm_backproject and pm_point_cloud (include/pm/imaging.h); included by pm_stages.hip
// alone.  The arithmetic and the per-thread bodies (backproject_four, cloud_item, cloud_store) are pm_cloud_body.hpp's,
// the definition is tests/pointcloud_ref.py (DESIGN.md sections 8b, 8c).
//
// k_backproject: one pass, 4 B in and 12 B out per pixel.  A thread owns four consecutive pixels of a row; their 48 output
// bytes leave as three 16-byte stores where the address is 16-byte aligned and the row holds all four, float by float
// otherwise (row tails, an unaligned destination, rows of an image whose width is no multiple of 4) -- the rule of
// rectify_four's float image.
//
// The compacted cloud is three launches without a wait between workgroups:
//   k_cloud_count    a block of kCloudBlock threads takes kCloudBlock consecutive ITEMS (the pixels of the stride grid in
//                    row-major order, one per thread); each wavefront ballots the filter predicate and counts its bits,
//                    the four counts meet in LDS, the block writes their sum;
//   k_cloud_offsets  ONE block turns the per-block counts into exclusive offsets in place, kCloudScanThreads at a time with
//                    a running carry, and writes the total;
//   k_cloud_scatter  the same predicate again; slot = block offset + counts of the wavefronts in front + the lane's rank
//                    under the ballot mask (v_mbcnt); stored only where slot < capacity.
// The order of the output is this arithmetic, never an atomic: row-major, reproducible, bit-comparable.  Predicate and
// point are cloud_item() in both launches, and cloud_item() is cloud_point() + cloud_counts(): what k_backproject runs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_cloud_body.hpp"

namespace pm {

constexpr int kCloudBlockX = 64;         // k_backproject: threads along a row (256 pixels)
constexpr int kCloudBlockY = 4;          // ... and rows per block
constexpr int kCloudBlock = 256;         // items per block of the count / scatter launches: four wavefronts
constexpr int kCloudScanThreads = 1024;  // block counts the offsets kernel takes per pass

// grid = (ceil(cols / 256), ceil(rows / 4)), block = (64, 4)
__global__ void __launch_bounds__(kCloudBlockX * kCloudBlockY) k_backproject(BackprojectArgs a) {
  const int x4 = (int)(blockIdx.x * kCloudBlockX + threadIdx.x) * 4;
  const int y = (int)(blockIdx.y * kCloudBlockY + threadIdx.y);
  if (x4 >= a.cols || y >= a.rows) return;
  backproject_four(a, x4, y);
}

// The predicate of the thread's item as a 64-bit ballot; every thread of the block gets here (no early return in front of
// a ballot or a barrier).
__device__ __forceinline__ bool cloud_thread_item(const CloudArgs& a, int* x, int* y, float p[3]) {
  const long long item = (long long)blockIdx.x * kCloudBlock + threadIdx.x;
  *x = *y = 0;
  p[0] = p[1] = p[2] = 0.f;
  return item < a.items && cloud_item(a, item, x, y, p);
}

// grid = ceil(items / kCloudBlock), block = kCloudBlock.  counts[blockIdx.x] = counted items of the block.
__global__ void __launch_bounds__(kCloudBlock) k_cloud_count(CloudArgs a, int* __restrict__ counts) {
  __shared__ int wave_count[kCloudBlock / 64];
  int x, y;
  float p[3];
  const bool counted = cloud_thread_item(a, &x, &y, p);
  const unsigned long long mask = __ballot(counted);
  if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = __popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kCloudBlock / 64; ++w) sum += wave_count[w];
    counts[blockIdx.x] = sum;
  }
}

// grid = 1, block = kCloudScanThreads.  counts[0 .. n) -> exclusive offsets in place; *total (and *d_count where given)
// = their sum.  n > kCloudScanThreads: further passes, each starting from the carry of the one before.
__global__ void __launch_bounds__(kCloudScanThreads) k_cloud_offsets(int* __restrict__ counts, int n, int* __restrict__ total,
                                                                     int* __restrict__ d_count) {
  constexpr int kWaves = kCloudScanThreads / 64;
  __shared__ int wave_sum[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += kCloudScanThreads) {  // uniform trip count: shuffles and barriers see every thread
    const int i = base + (int)threadIdx.x;
    const int v = i < n ? counts[i] : 0;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int s = wave_sum[w];
      before += w < wave ? s : 0;
      all += s;
    }
    if (i < n) counts[i] = carry + before + (incl - v);
    carry += all;
    __syncthreads();  // wave_sum is rewritten by the next pass
  }
  if (threadIdx.x == 0) {
    *total = carry;
    if (d_count) *d_count = carry;
  }
}

// grid and block as k_cloud_count; offsets: what k_cloud_offsets left.
__global__ void __launch_bounds__(kCloudBlock) k_cloud_scatter(CloudArgs a, const int* __restrict__ offsets, CloudStreams s) {
  __shared__ int wave_count[kCloudBlock / 64];
  int x, y;
  float p[3];
  const bool counted = cloud_thread_item(a, &x, &y, p);
  const unsigned long long mask = __ballot(counted);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wave_count[wave] = __popcll(mask);
  __syncthreads();
  int slot = offsets[blockIdx.x];
#pragma unroll
  for (int w = 0; w < kCloudBlock / 64; ++w) slot += w < wave ? wave_count[w] : 0;
  // the lane's rank among the set bits of the mask below it
  slot += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
  if (counted && slot < s.capacity) cloud_store(a, s, slot, x, y, p);
}

}  // namespace pm
