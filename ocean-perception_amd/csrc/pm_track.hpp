// pm_track.hpp -- the kernels of pm_track_features (include/pm/imaging.h); included by pm_stages.hip alone.  The scalar pieces
// (score, eligibility, prediction, the SAD of a candidate, the key, sub-pixel, the record) are pm_track_body.hpp's, the
// definition is tests/motion_ref.py.
//
// Three launches, none of which waits for another workgroup and none of which uses an atomic:
//   k_track_select   one workgroup per cell.  It stages the cell with its 4-pixel halo of the old image in LDS, forms the Sobel
//                    pairs of the cell with a 3-pixel halo there, then every thread scores pixels of the cell (49 LDS reads
//                    of a packed pair each) and keeps the best (score, index) it saw; a tree in LDS reduces the 256 pairs to
//                    the cell's feature: its pixel index y cols + x, or -1.
//   k_track_compact  ONE workgroup turns the per-cell results into the feature list in cell order: per pass of 1024 cells a
//                    ballot per wavefront, the wavefronts' counts in LDS, the lane's rank under the ballot mask (v_mbcnt),
//                    and a running carry -- k_cloud_offsets' scheme.  It writes the total.
//   k_track_match    one workgroup per record.  The template (at most 15 rows of 16 bytes) and the search region
//                    ((2s + 2p + 1)^2 bytes, at most 63 rows of 72) are built in LDS as words; lanes take candidates in
//                    strides of 256; a candidate's SAD runs four bytes at a time (v_alignbyte_b32 + v_sad_u8) and is kept as
//                    16 bits in an LDS table; the workgroup reduces the key sad << 12 | index to its minimum, then the
//                    smallest SAD at Chebyshev distance >= 2 from it; thread 0 reads the two parabolas from the table and
//                    stores the record.
// Only integers cross lanes, and nothing crosses workgroups but the feature list, so every output is a pure function of
// the inputs.  Every thread of every block reaches every barrier and every ballot: what a block skips, it skips under a
// block-uniform condition around the work, never around a barrier.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pm_track_body.hpp"

namespace pm {

constexpr int kTrackBlock = 256;           // k_track_select, k_track_match: four wavefronts
constexpr int kTrackCompactThreads = 1024;  // cells k_track_compact takes per pass
constexpr int kTrackTileMax = kTrackMaxCell + 2 * kTrackHalo;  // 72
constexpr int kTrackGradMax = kTrackMaxCell + 2 * 3;           // 70
static_assert(kTrackMaxCandidates <= 4096, "a candidate's index takes the low 12 bits of its key");

struct TrackSelectArgs {
  TrackOpt opt;
  const uint8_t* old;
  const float* disp;
  int rows, cols;
  int* cell_best;  // [gridDim.y][gridDim.x]
};

// grid = (ceil(cols / cell), ceil(rows / cell)), block = 256
__global__ void __launch_bounds__(kTrackBlock) k_track_select(TrackSelectArgs a) {
  __shared__ uint8_t tile[kTrackTileMax * kTrackTileMax];
  __shared__ TrackGrad grad[kTrackGradMax * kTrackGradMax];
  __shared__ long long red_score[kTrackBlock];
  __shared__ int red_index[kTrackBlock];
  const int cell = a.opt.cell, tp = cell + 2 * kTrackHalo, gp = cell + 6;
  const int x0 = (int)blockIdx.x * cell, y0 = (int)blockIdx.y * cell;
  const int tid = (int)threadIdx.x;
  for (int i = tid; i < tp * tp; i += kTrackBlock) {
    const int ly = i / tp, lx = i - ly * tp;
    const int gx = x0 - kTrackHalo + lx, gy = y0 - kTrackHalo + ly;
    const bool inside = gx >= 0 && gx < a.cols && gy >= 0 && gy < a.rows;
    tile[i] = inside ? a.old[(size_t)gy * a.cols + gx] : (uint8_t)0;
  }
  __syncthreads();
  for (int i = tid; i < gp * gp; i += kTrackBlock) {
    const int ly = i / gp, lx = i - ly * gp;
    grad[i] = track_sobel(tile, tp, lx + 1, ly + 1);
  }
  __syncthreads();
  long long best_score = 0;
  int best_index = -1;
  for (int i = tid; i < cell * cell; i += kTrackBlock) {
    const int py = i / cell, px = i - py * cell;
    const int x = x0 + px, y = y0 + py;
    if (x >= a.cols || y >= a.rows) continue;
    const int index = y * a.cols + x;
    if (!track_eligible(a.opt, a.rows, a.cols, x, y, a.disp[index])) continue;
    const long long score = track_score(grad, gp, px + 3, py + 3);
    if (score >= a.opt.min_score && track_better(score, index, best_score, best_index)) best_score = score, best_index = index;
  }
  red_score[tid] = best_score;
  red_index[tid] = best_index;
  __syncthreads();
  for (int half = kTrackBlock / 2; half > 0; half >>= 1) {  // uniform trip count
    if (tid < half && track_better(red_score[tid + half], red_index[tid + half], red_score[tid], red_index[tid])) {
      red_score[tid] = red_score[tid + half];
      red_index[tid] = red_index[tid + half];
    }
    __syncthreads();
  }
  if (tid == 0) a.cell_best[blockIdx.y * gridDim.x + blockIdx.x] = red_index[0];
}

// grid = 1, block = 1024.  feat[0 .. *total): the entries >= 0 of cell_best[0 .. n) in order.
__global__ void __launch_bounds__(kTrackCompactThreads) k_track_compact(const int* __restrict__ cell_best, int n,
                                                                         int* __restrict__ feat, int* __restrict__ total,
                                                                         int* __restrict__ d_count) {
  constexpr int kWaves = kTrackCompactThreads / 64;
  __shared__ int wave_count[kWaves];
  const int wave = (int)threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += kTrackCompactThreads) {  // uniform trip count
    const int i = base + (int)threadIdx.x;
    const int index = i < n ? cell_best[i] : -1;
    const bool has = index >= 0;
    const unsigned long long mask = __ballot(has);
    if ((threadIdx.x & 63) == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int c = wave_count[w];
      before += w < wave ? c : 0;
      all += c;
    }
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    if (has) feat[carry + before + rank] = index;  // at most one entry per cell: inside feat[0 .. n)
    carry += all;
    __syncthreads();  // wave_count is rewritten by the next pass
  }
  if (threadIdx.x == 0) {
    *total = carry;
    if (d_count) *d_count = carry;
  }
}

struct TrackMatchArgs {
  TrackOpt opt;
  CloudCam cam;
  double R[9], t[3];
  const uint8_t* old;
  const float* disp;
  const uint8_t* img;  // the new left image
  int rows, cols;
  const int* feat;
  const int* total;
  pm_track* tracks;  // record blockIdx.x; the grid holds no more blocks than the capacity
};

// the minimum of v over the block; `slots`: one word per wavefront.  Every thread calls it.
__device__ __forceinline__ unsigned track_block_min(unsigned v, unsigned* slots) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned other = (unsigned)__shfl_xor((int)v, o);
    v = other < v ? other : v;
  }
  __syncthreads();  // the slots may still be read from the call before
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned m = slots[0];
#pragma unroll
  for (int w = 1; w < kTrackBlock / 64; ++w) m = slots[w] < m ? slots[w] : m;
  return m;
}

// grid = min(cells, capacity), block = 256
__global__ void __launch_bounds__(kTrackBlock) k_track_match(TrackMatchArgs a) {
  __shared__ unsigned tmpl[(2 * kTrackMaxPatch + 1) * kTrackTmplPitchW];
  __shared__ unsigned region[kTrackMaxRegion * kTrackMaxRegionPitchW];
  __shared__ uint16_t table[kTrackMaxCandidates];
  __shared__ unsigned slots[kTrackBlock / 64];
  const int tid = (int)threadIdx.x, k = (int)blockIdx.x;
  const int p = a.opt.p, s = a.opt.s;
  const bool live = k < *a.total;  // block-uniform
  int x = 0, y = 0, iu = 0, iv = 0;
  float d = 1.f;
  bool predicted = false;
  if (live) {
    const int index = a.feat[k];
    y = index / a.cols, x = index - y * a.cols;
    d = a.disp[index];
    predicted = track_predict(a.cam, a.R, a.t, d, x, y, &iu, &iv);  // the same in every thread
  }
  const int n = 2 * p + 1, width = 2 * s + n, pitch_w = track_region_pitch(p, s), n1 = 2 * s + 1;
  if (predicted) {
    for (int i = tid; i < n * kTrackTmplPitchW; i += kTrackBlock)
      tmpl[i] = track_tmpl_word(a.old, a.cols, x, y, p, i % kTrackTmplPitchW, i / kTrackTmplPitchW);
    for (int i = tid; i < width * pitch_w; i += kTrackBlock) {
      const int ly = i / pitch_w;
      region[i] = track_region_word(a.img, a.rows, a.cols, iu - s - p, iv - s - p, width, i - ly * pitch_w, ly);
    }
  }
  __syncthreads();
  unsigned key = kTrackNoKey;
  if (predicted)
    for (int c = tid; c < n1 * n1; c += kTrackBlock) {
      const int ey = c / n1, ex = c - ey * n1;
      unsigned sad = kTrackNoSad;
      if (track_counts(a.rows, a.cols, p, iu - s + ex, iv - s + ey)) {
        sad = track_sad(tmpl, region, pitch_w, p, ex, ey);
        const unsigned mine = track_key(sad, c);
        key = mine < key ? mine : key;
      }
      table[c] = (uint16_t)sad;
    }
  key = track_block_min(key, slots);  // its barriers also publish the table
  unsigned second = kTrackNoSad;
  if (key != kTrackNoKey)
    for (int c = tid; c < n1 * n1; c += kTrackBlock) {
      const unsigned sad = table[c];
      if (sad < second && track_far(c, (int)(key & 4095u), n1)) second = sad;
    }
  second = track_block_min(second, slots);
  if (live && tid == 0) {
    pm_track r;
    if (predicted)
      track_finish(a.opt, table, iu, iv, key, second, x, y, d, &r);
    else
      track_unpredicted(x, y, d, &r);
    a.tracks[k] = r;
  }
}

}  // namespace pm
