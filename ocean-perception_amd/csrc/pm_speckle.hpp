// pm_speckle.hpp -- the kernels of pm_filter_speckles (include/pm/imaging.h); included by pm_stages.hip alone.  What a
// thread does is pm_speckle_body.hpp's, the definition is tests/speckle_ref.py.
//
// Four launches on one stream; the boundary between two of them is the only thing a workgroup ever waits for:
//   k_speckle_local    labels one 64 x 16 tile in LDS and writes working labels (the image index of the tile-local root)
//                      and the tile-local components' pixel counts at their roots
//   k_speckle_merge    one thread per pixel of a tile's first column or row: unites across the border
//   k_speckle_flatten  one thread per pixel: its root; tile-local counts move to the root
//   k_speckle_apply    one thread per pixel: out, labels, sizes; the removed count, one integer atomic per block
// Termination is structural: every parent is a strictly smaller index (the invariant at the head of the body header), so
// every loop strictly decreases; no kernel spins on a value another workgroup has yet to write; no thread returns in front
// of a ballot or a barrier.  Across workgroups only integer min and integer add are used, so every output is a pure
// function of the input.  Vector atomics and plain C++ only, no inline assembly.
#pragma once

#include <hip/hip_runtime.h>

#include "pm_speckle_body.hpp"

namespace pm {

constexpr int kSpeckleBlock = 256;  // threads of the three per-item launches

// LDS of the workgroup: every access that may run beside a writer is an atomic of workgroup scope (a ds_ instruction each)
struct SpeckleLdsMem {
  __device__ int load(const int* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ void store(int* p, int v) const { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ int atomic_min(int* p, int v) const {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ void atomic_add(int* p, int v) const {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};

// Global memory that other workgroups write in the same launch.  Loads are relaxed atomics of agent scope: a plain load may
// be served from this CU's L1, which no other CU's store refreshes, or from another XCD's view of the line.  A stale parent
// would still obey the invariant; correctness rests on what the atomics return alone.
struct SpeckleGlobalMem {
  __device__ int load(const int* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ void store(int* p, int v) const { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ int atomic_min(int* p, int v) const {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ void atomic_add(int* p, int v) const {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// grid = tiles_x * tiles_y (one dimension: no 65535-row limit), block = (kSpeckleTileCols, kSpeckleTileRows): a wavefront is
// a tile row, so a ballot is that row's mask.  Every thread reaches all four barriers; cells outside the image are invalid.
__global__ void __launch_bounds__(kSpeckleTileCells) k_speckle_local(SpeckleArgs a, int tiles_x) {
  __shared__ float tile[kSpeckleTileCells];
  __shared__ int lab[kSpeckleTileCells];
  __shared__ int cnt[kSpeckleTileCells];
  __shared__ unsigned long long row_starts[kSpeckleTileRows];
  const SpeckleLdsMem lds;
  const int lane = (int)threadIdx.x, row = (int)threadIdx.y, cell = row * kSpeckleTileCols + lane;
  const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * kSpeckleTileCols;
  const int y0 = (int)(blockIdx.x / (unsigned)tiles_x) * kSpeckleTileRows;
  const int x = x0 + lane, y = y0 + row;
  const bool inside = x < a.cols && y < a.rows;
  const float d = inside ? a.disp[(size_t)y * a.cols + x] : 0.f;
  tile[cell] = d;
  cnt[cell] = 0;
  __syncthreads();
  // runs along the row: no iteration, the run's first lane is a bit scan of the ballot
  const bool valid = speckle_valid(d);
  const bool joined_left = lane > 0 && speckle_joined(d, tile[cell - 1], a.max_diff);
  const unsigned long long starts = __ballot(!joined_left);
  lab[cell] = speckle_tile_init(row, lane, valid, starts);
  if (lane == 0) row_starts[row] = starts;
  const bool joined_up = row > 0 && speckle_joined(d, tile[cell - kSpeckleTileCols], a.max_diff);
  const unsigned long long up = __ballot(joined_up);
  __syncthreads();
  // rows: union-find in LDS.  Each union's loop strictly decreases (speckle_union) and waits for no other thread.
  if (row > 0 && ((speckle_link_mask(up, starts, row_starts[row - 1]) >> lane) & 1)) speckle_tile_link(lds, lab, row, lane);
  __syncthreads();
  const int root = speckle_tile_flatten(lds, lab, cnt, row, lane, valid, starts);
  __syncthreads();
  if (inside) speckle_tile_store(a, x0, y0, row, lane, root, cnt);
}

// grid = ceil(speckle_merge_items / kSpeckleBlock)
__global__ void __launch_bounds__(kSpeckleBlock) k_speckle_merge(SpeckleArgs a, long long items) {
  const long long item = (long long)blockIdx.x * kSpeckleBlock + threadIdx.x;
  if (item < items) speckle_merge_item(SpeckleGlobalMem(), a, item);
}

// grid = ceil(pixels / kSpeckleBlock)
__global__ void __launch_bounds__(kSpeckleBlock) k_speckle_flatten(SpeckleArgs a, int pixels) {
  const long long p = (long long)blockIdx.x * kSpeckleBlock + threadIdx.x;
  if (p < pixels) speckle_flatten_item(SpeckleGlobalMem(), a, (int)p);
}

// grid = ceil(pixels / kSpeckleBlock); *removed was cleared on the stream in front of the launch
__global__ void __launch_bounds__(kSpeckleBlock) k_speckle_apply(SpeckleArgs a, SpeckleOut o, int pixels, int* removed) {
  __shared__ int block_removed;
  if (threadIdx.x == 0) block_removed = 0;
  __syncthreads();
  const long long p = (long long)blockIdx.x * kSpeckleBlock + threadIdx.x;
  const bool gone = p < pixels && speckle_apply_item(a, o, (int)p);  // no thread leaves in front of the ballot
  const unsigned long long mask = __ballot(gone);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&block_removed, __popcll(mask));
  __syncthreads();
  if (threadIdx.x == 0 && block_removed) atomicAdd(removed, block_removed);
}

}  // namespace pm
