// pm_guided.hpp -- the fast guided filter with a one-channel guide (include/pm/imaging.h: pm_fast_guided_filter,
// pm_estimate_illuminant_range_guided) and the pixel gather (pm_gather_pixels).  Restates
// src/vehicle/imaging/fast_guided_filter.cpp:68-123, :207-233; the definition the kernels are held to bit for bit is
// tests/guided_ref.py.
//
// Two halves of very different size:
//   coarse (rows/s x cols/s, 90 x 160 at 720p with s = 8): four launches, launch-latency bound
//     k_gf_box_rows<true>   nearest-neighbour gather of guide / src, the product planes I, I*I, p_c, I*p_c, and the
//                           ordered binary64 row sums of the k taps of every output; the row is staged in LDS
//     k_gf_box_cols_ab      the k row sums top to bottom in binary64, one rounding to binary32, then the a / b algebra
//     k_gf_box_rows<false>  row sums of the a_c / b_c planes
//     k_gf_box_cols_mean    mean_a / mean_b, written interleaved ([y][x][c][a, b]) for the last kernel
//   full resolution: k_gf_apply reads the guide once (4 B / px), interpolates mean_a / mean_b of every channel from
//     the coarse planes (L2 resident) and writes channels x 4 B / px; bound: HBM.
// The box sums are NOT sliding or prefix sums: the definition fixes the order of the binary64 additions (left to right,
// then top to bottom), and any other order changes the rounding.  No FMA (the build uses -ffp-contract=off), float
// division correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pm {

// cv::borderInterpolate(p, n, BORDER_REFLECT_101), with its repeated reflection when |p| >= n
__device__ __forceinline__ int gf_reflect101(int p, int n) {
  if (n == 1) return 0;
  while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}

// cv::resize INTER_NN: source index of destination index d; inv = 1.0 / ((double)dst / src)
__device__ __forceinline__ int gf_nn_index(int d, double inv, int src) {
  const int i = (int)floor((double)d * inv);
  return i < src - 1 ? i : src - 1;
}

// cv::resize INTER_LINEAR on floats, one axis: left tap and the binary32 weight of the right tap
__device__ __forceinline__ void gf_linear_axis(int d, double scale, int src, int* i0, int* i1, float* w) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int i = (int)floorf(f);
  f = f - (float)i;
  if (i < 0) {
    i = 0;
    f = 0.f;
  }
  if (i >= src - 1) {
    i = src - 1;
    f = 0.f;
  }
  *i0 = i;
  *i1 = i + 1 < src ? i + 1 : src - 1;
  *w = f;
}

struct GfShape {
  int rows, cols;    // full resolution
  int crows, ccols;  // coarse: rows / s, cols / s
  int channels;      // of src, 1..4
  int k;             // box size 2 * (r / s) + 1
  double inv_y, inv_x;  // 1.0 / ((double)crows / rows), 1.0 / ((double)ccols / cols): INTER_NN down
  double up_y, up_x;    // 1.0 / ((double)rows / crows), 1.0 / ((double)cols / ccols): INTER_LINEAR up
};

// Ordered row sums.  grid = (coarse rows, planes), one block per (row, plane); the plane's row is staged in LDS
// (ccols floats, dynamic), then every thread adds the k taps of its outputs left to right in binary64.
// GATHER: the planes are computed from the full-resolution images: plane 0 = I, 1 = I * I, 2 + 2c = p_c, 3 + 2c = I * p_c
// (binary32 products, cv::Mat::mul).  Otherwise `planes` holds them: [plane][crows][ccols] floats.
template <bool GATHER>
__global__ void __launch_bounds__(256) k_gf_box_rows(const float* __restrict__ guide, const float* __restrict__ src,
                                                     const float* __restrict__ planes, GfShape g,
                                                     double* __restrict__ rowsum) {
  extern __shared__ float gf_row[];
  const int y = blockIdx.x, plane = blockIdx.y;
  const size_t cpx = (size_t)g.crows * g.ccols;
  if (GATHER) {
    const int sy = gf_nn_index(y, g.inv_y, g.rows);
    const int c = plane >= 2 ? (plane - 2) >> 1 : 0;
    for (int x = threadIdx.x; x < g.ccols; x += blockDim.x) {
      const size_t at = (size_t)sy * g.cols + gf_nn_index(x, g.inv_x, g.cols);
      const float I = guide[at];
      float v;
      if (plane == 0)
        v = I;
      else if (plane == 1)
        v = I * I;
      else if (plane & 1)
        v = I * src[at * g.channels + c];
      else
        v = src[at * g.channels + c];
      gf_row[x] = v;
    }
  } else {
    const float* row = planes + (size_t)plane * cpx + (size_t)y * g.ccols;
    for (int x = threadIdx.x; x < g.ccols; x += blockDim.x) gf_row[x] = row[x];
  }
  __syncthreads();
  const int half = g.k >> 1;
  double* out = rowsum + (size_t)plane * cpx + (size_t)y * g.ccols;
  for (int x = threadIdx.x; x < g.ccols; x += blockDim.x) {
    double acc = 0.0;
    if (x - half >= 0 && x + half < g.ccols) {  // interior: no reflection
      for (int i = x - half; i <= x + half; ++i) acc += (double)gf_row[i];
    } else {
      for (int i = x - half; i <= x + half; ++i) acc += (double)gf_row[gf_reflect101(i, g.ccols)];
    }
    out[x] = acc;
  }
}

// the k row sums of N planes at (y, x), top to bottom in binary64, times 1 / k^2, one rounding each (N independent chains)
template <int N>
__device__ __forceinline__ void gf_col_sums(const double* const (&p)[N], const GfShape& g, int y, int x, float (&out)[N]) {
  const int half = g.k >> 1;
  double acc[N];
#pragma unroll
  for (int n = 0; n < N; ++n) acc[n] = 0.0;
  for (int j = y - half; j <= y + half; ++j) {
    const size_t at = (size_t)gf_reflect101(j, g.crows) * g.ccols + x;
#pragma unroll
    for (int n = 0; n < N; ++n) acc[n] += p[n][at];
  }
  const double norm = 1.0 / ((double)g.k * (double)g.k);
#pragma unroll
  for (int n = 0; n < N; ++n) out[n] = (float)(acc[n] * norm);
}

// Column sums of the first box pass and the algebra of fast_guided_filter.cpp:101-115.  grid = (coarse pixels / 128,
// channels): a thread owns one coarse pixel of one channel and carries four independent binary64 chains (mean_I,
// mean_II, mean_p, mean_Ip; the first two are recomputed per channel, which costs less than a launch).
// ab: [2 * channels][crows][ccols] floats, plane 2c = a_c, 2c + 1 = b_c.
__global__ void __launch_bounds__(128) k_gf_box_cols_ab(const double* __restrict__ rowsum, GfShape g, float eps,
                                                        float* __restrict__ ab) {
  const size_t cpx = (size_t)g.crows * g.ccols;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cpx) return;
  const int c = blockIdx.y;
  const int y = (int)(i / g.ccols), x = (int)(i % g.ccols);
  const double* const p[4] = {rowsum, rowsum + cpx, rowsum + (size_t)(2 + 2 * c) * cpx, rowsum + (size_t)(3 + 2 * c) * cpx};
  float m[4];
  gf_col_sums<4>(p, g, y, x, m);
  const float mean_I = m[0], mean_II = m[1], mean_p = m[2], mean_Ip = m[3];
  const float var_I = mean_II - mean_I * mean_I;
  const float cov_Ip = mean_Ip - mean_I * mean_p;
  const float a = cov_Ip / (var_I + eps);
  const float b = mean_p - a * mean_I;
  ab[(size_t)(2 * c) * cpx + i] = a;
  ab[(size_t)(2 * c + 1) * cpx + i] = b;
}

// Column sums of the second box pass: mean_a_c, mean_b_c, interleaved as mean[(y * ccols + x) * 2 * channels + 2c + {0, 1}].
__global__ void __launch_bounds__(128) k_gf_box_cols_mean(const double* __restrict__ rowsum, GfShape g,
                                                          float* __restrict__ mean) {
  const size_t cpx = (size_t)g.crows * g.ccols;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cpx) return;
  const int c = blockIdx.y;
  const int y = (int)(i / g.ccols), x = (int)(i % g.ccols);
  const double* const p[2] = {rowsum + (size_t)(2 * c) * cpx, rowsum + (size_t)(2 * c + 1) * cpx};
  float m[2];
  gf_col_sums<2>(p, g, y, x, m);
  float* out = mean + (i * g.channels + c) * 2;
  out[0] = m[0];
  out[1] = m[1];
}

// One full-resolution pixel: mean_a / mean_b of every channel interpolated from the coarse planes (horizontal pass,
// then vertical, binary32, unfused: cv::resize INTER_LINEAR), out_c = (mean_a_c * I + mean_b_c) * scale.
template <int CH>
__device__ __forceinline__ void gf_apply_pixel(const float* __restrict__ mean, const GfShape& g, int y, int x, float I,
                                               float scale, float out[CH]) {
  int x0, x1, y0, y1;
  float fx, fy;
  gf_linear_axis(x, g.up_x, g.ccols, &x0, &x1, &fx);
  gf_linear_axis(y, g.up_y, g.crows, &y0, &y1, &fy);
  const float gx = 1.f - fx, gy = 1.f - fy;
  const float2* t00 = (const float2*)mean + ((size_t)y0 * g.ccols + x0) * CH;
  const float2* t01 = (const float2*)mean + ((size_t)y0 * g.ccols + x1) * CH;
  const float2* t10 = (const float2*)mean + ((size_t)y1 * g.ccols + x0) * CH;
  const float2* t11 = (const float2*)mean + ((size_t)y1 * g.ccols + x1) * CH;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const float2 v00 = t00[c], v01 = t01[c], v10 = t10[c], v11 = t11[c];
    const float a_top = v00.x * gx + v01.x * fx, a_bot = v10.x * gx + v11.x * fx;
    const float b_top = v00.y * gx + v01.y * fx, b_bot = v10.y * gx + v11.y * fx;
    const float mean_a = a_top * gy + a_bot * fy;
    const float mean_b = b_top * gy + b_bot * fy;
    out[c] = (mean_a * I + mean_b) * scale;
  }
}

// Full-resolution pass.  vec_ok (guide and dst 16-byte aligned): a lane takes four consecutive pixels of the flattened
// image -- one float4 of the guide in, CH float4 out; otherwise, and for the last n_px % 4 pixels, one pixel per lane.
template <int CH>
__global__ void __launch_bounds__(256) k_gf_apply(const float* __restrict__ guide, const float* __restrict__ mean,
                                                  GfShape g, float scale, float* __restrict__ dst, int vec_ok) {
  const size_t n_px = (size_t)g.rows * g.cols;
  const size_t n4 = vec_ok ? n_px / 4 : 0;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (size_t)gridDim.x * blockDim.x) {
    const float4 I4 = ((const float4*)guide)[q];
    const float Iv[4] = {I4.x, I4.y, I4.z, I4.w};
    int y = (int)((q * 4) / g.cols), x = (int)((q * 4) % g.cols);
    float px[4 * CH];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      gf_apply_pixel<CH>(mean, g, y, x, Iv[k], scale, px + k * CH);
      if (++x == g.cols) {
        x = 0;
        ++y;
      }
    }
    float4* o = (float4*)dst + q * CH;
#pragma unroll
    for (int v = 0; v < CH; ++v) o[v] = make_float4(px[4 * v], px[4 * v + 1], px[4 * v + 2], px[4 * v + 3]);
  }
  for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_px; i += (size_t)gridDim.x * blockDim.x) {
    float px[CH];
    gf_apply_pixel<CH>(mean, g, (int)(i / g.cols), (int)(i % g.cols), guide[i], scale, px);
#pragma unroll
    for (int c = 0; c < CH; ++c) dst[i * CH + c] = px[c];
  }
}

// pm_gather_pixels: out[i][c] = img[y_i][x_i][c].  An entry outside the image is not clamped: nothing is written for it
// and *bad is raised (the host reports PM_ERR_INVALID_ARG).
__global__ void __launch_bounds__(256) k_gather_pixels(const float* __restrict__ img, int rows, int cols, int channels,
                                                       const int32_t* __restrict__ xy, int n, float* __restrict__ out,
                                                       unsigned* bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = xy[2 * i], y = xy[2 * i + 1];
  if (x < 0 || y < 0 || x >= cols || y >= rows) {
    atomicOr(bad, 1u);
    return;
  }
  const float* p = img + ((size_t)y * cols + x) * channels;
  for (int c = 0; c < channels; ++c) out[(size_t)i * channels + c] = p[c];
}

}  // namespace pm
