// pm_imaging.hip -- C-ABI implementation of the imaging rows of include/pm/imaging.h: range and the range-dependent
// corrections, the stereo-ready enhancement, the guided filter and the pixel gather, undistortion
// and rectification in front of Match(), pm_stereo_rectify, and the device-buffer helpers.  The stages that read a
// finished disparity map are pm_stages.hip's.  A separate translation unit: it reaches the handle only through
// pm_internal.hpp (device, stream, error text, one opaque state slot); the state in that slot is
// pm_imaging_state.hpp's, shared with pm_stages.hip and released here.
#include "pm/imaging.h"

#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pm_enhance.hpp"
#include "pm_guided.hpp"
#include "pm_imaging.hpp"
#include "pm_imaging_state.hpp"
#include "pm_rectify.hpp"
#include "pm_tune.hpp"

using namespace pm;

void pm_internal::release_imaging(pm_handle* h) {
  void** slot = pm_internal::imaging_slot(h);
  delete static_cast<ImagingState*>(*slot);
  *slot = nullptr;
}

// ---- pm/imaging.h: disparity -> range -> range-dependent correction -----------------------------
namespace {

int imaging_begin(pm_handle* h, const char* what, const void* a, const void* b, int rows, int cols) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (!a || !b || rows <= 0 || cols <= 0) {
    set_err(h, "%s: null pointer or empty image", what);
    return PM_ERR_INVALID_ARG;
  }
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  if (!state_of(h)) {
    set_err(h, "%s: out of host memory", what);
    return PM_ERR_NOMEM;
  }
  if (!state_of(h)->img_scalars) PM_HIP(h, state_of(h)->img_scalars.alloc_zeroed(sizeof(unsigned) * 4, pm_internal::stream(h)));
  return PM_OK;
}

inline dim3 stream_grid(size_t n_items) {  // grid-stride: enough blocks to fill 256 CUs a few times over
  size_t b = (n_items + 255) / 256;
  if (b > 256 * 16) b = 256 * 16;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

inline dim3 reduce_grid(size_t n_items) {  // reductions: one atomic per block, so no more blocks than fill the chip
  size_t b = (n_items + 255) / 256;
  if (b > 256 * 8) b = 256 * 8;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

BackscatterParams backscatter_params(const float B[3], const float beta_B[3]) {
  BackscatterParams bp{};
  for (int c = 0; c < 3; ++c) {
    bp.B[c] = B ? B[c] : 0.f;
    bp.beta_B[c] = beta_B ? beta_B[c] : 0.f;
  }
  return bp;
}
AttenuationParams attenuation_params(const float X[12]) {
  AttenuationParams ap{};
  for (int c = 0; c < 3; ++c) {
    ap.a[c] = X ? X[c] : 0.f;
    ap.b[c] = X ? X[3 + c] : 0.f;
    ap.c[c] = X ? X[6 + c] : 0.f;
    ap.d[c] = X ? X[9 + c] : 0.f;
  }
  return ap;
}

}  // namespace

int pm_disp_to_range(pm_handle* h, const float* d_disp, int rows, int cols, double fx, double baseline,
                     float* d_range) {
  if (int rc = imaging_begin(h, "pm_disp_to_range", d_disp, d_range, rows, cols)) return rc;
  const size_t n = (size_t)rows * cols;
  hipLaunchKernelGGL(k_disp_to_range, stream_grid(n), dim3(256), 0, pm_internal::stream(h), d_disp, n, fx * baseline, d_range,
                     (unsigned*)nullptr);
  return launch_check(h, "disp_to_range");
}

int pm_remove_backscatter(pm_handle* h, const float* d_bgr, const float* d_range, int rows, int cols,
                          const float B[3], const float beta_B[3], float* d_out) {
  if (int rc = imaging_begin(h, "pm_remove_backscatter", d_bgr, d_range, rows, cols)) return rc;
  if (!B || !beta_B || !d_out) {
    set_err(h, "pm_remove_backscatter: null parameter");
    return PM_ERR_INVALID_ARG;
  }
  const size_t n = (size_t)rows * cols;
  const int vec = aligned16(d_bgr) && aligned16(d_range) && aligned16(d_out);
  hipLaunchKernelGGL((k_range_enhance<1>), stream_grid(n / 4 + 1), dim3(256), 0, pm_internal::stream(h), d_bgr, d_range, n, 0.0,
                     backscatter_params(B, beta_B), attenuation_params(nullptr), (const unsigned*)state_of(h)->img_scalars,
                     (float*)nullptr, d_out, vec);
  return launch_check(h, "remove_backscatter");
}

int pm_correct_attenuation(pm_handle* h, const float* d_bgr, const float* d_range, int rows, int cols,
                           const float X[12], float* d_out) {
  if (int rc = imaging_begin(h, "pm_correct_attenuation", d_bgr, d_range, rows, cols)) return rc;
  if (!X || !d_out) {
    set_err(h, "pm_correct_attenuation: null parameter");
    return PM_ERR_INVALID_ARG;
  }
  const size_t n = (size_t)rows * cols;
  PM_HIP(h, hipMemsetAsync(state_of(h)->img_scalars, 0, sizeof(unsigned), pm_internal::stream(h)));
  hipLaunchKernelGGL(k_range_max, reduce_grid(n), dim3(256), 0, pm_internal::stream(h), d_range, n, state_of(h)->img_scalars);
  const int vec = aligned16(d_bgr) && aligned16(d_range) && aligned16(d_out);
  hipLaunchKernelGGL((k_range_enhance<2>), stream_grid(n / 4 + 1), dim3(256), 0, pm_internal::stream(h), d_bgr, d_range, n, 0.0,
                     backscatter_params(nullptr, nullptr), attenuation_params(X), (const unsigned*)state_of(h)->img_scalars,
                     (float*)nullptr, d_out, vec);
  return launch_check(h, "correct_attenuation");
}

int pm_range_enhance(pm_handle* h, const float* d_bgr, const float* d_disp, int rows, int cols, double fx,
                     double baseline, const float B[3], const float beta_B[3], const float X[12],
                     float* d_range_out, float* d_out) {
  if (int rc = imaging_begin(h, "pm_range_enhance", d_bgr, d_disp, rows, cols)) return rc;
  if (!B || !beta_B || !X || !d_out) {
    set_err(h, "pm_range_enhance: null parameter");
    return PM_ERR_INVALID_ARG;
  }
  const size_t n = (size_t)rows * cols;
  // pass 1: the largest range (CorrectAttenuation gives it to pixels without range); reads the disparity only
  PM_HIP(h, hipMemsetD32Async((hipDeviceptr_t)state_of(h)->img_scalars, 0x7f800000u, 1, pm_internal::stream(h)));
  hipLaunchKernelGGL(k_disp_min_positive, reduce_grid(n / 4 + 1), dim3(256), 0, pm_internal::stream(h), d_disp, n, state_of(h)->img_scalars,
                     aligned16(d_disp) ? 1 : 0);
  const int vec = aligned16(d_bgr) && aligned16(d_disp) && aligned16(d_out) && (!d_range_out || aligned16(d_range_out));
  hipLaunchKernelGGL((k_range_enhance<7>), stream_grid(n / 4 + 1), dim3(256), 0, pm_internal::stream(h), d_bgr, d_disp, n,
                     fx * baseline, backscatter_params(B, beta_B), attenuation_params(X),
                     (const unsigned*)state_of(h)->img_scalars, d_range_out, d_out, vec);
  return launch_check(h, "range_enhance");
}

int pm_compute_intensity(pm_handle* h, const float* d_bgr, int rows, int cols, float* d_gray) {
  if (int rc = imaging_begin(h, "pm_compute_intensity", d_bgr, d_gray, rows, cols)) return rc;
  const size_t n = (size_t)rows * cols;
  hipLaunchKernelGGL(k_intensity, stream_grid(n), dim3(256), 0, pm_internal::stream(h), d_bgr, n, d_gray);
  return launch_check(h, "intensity");
}

int pm_find_dark(pm_handle* h, const float* d_intensity, const float* d_range, int rows, int cols, float percentile,
                 uint8_t* d_mask, float* threshold) {
  if (int rc = imaging_begin(h, "pm_find_dark", d_intensity, d_range, rows, cols)) return rc;
  if (!d_mask || !threshold) {
    set_err(h, "pm_find_dark: null output");
    return PM_ERR_INVALID_ARG;
  }
  const size_t n = (size_t)rows * cols;
  // backscatter.cpp:41-78
  const float N = (float)(rows * cols);
  const int n_desired = (int)(percentile * N);
  auto count_at = [&](float thr, unsigned* out) -> int {
    PM_HIP(h, hipMemsetAsync(state_of(h)->img_scalars + 1, 0, sizeof(unsigned), pm_internal::stream(h)));
    hipLaunchKernelGGL(k_dark_count, reduce_grid(n), dim3(256), 0, pm_internal::stream(h), d_intensity, d_range, n, thr, d_mask,
                       state_of(h)->img_scalars + 1);
    PM_HIP(h, hipMemcpyAsync(out, state_of(h)->img_scalars + 1, sizeof(unsigned), hipMemcpyDeviceToHost, pm_internal::stream(h)));
    PM_HIP(h, hipStreamSynchronize(pm_internal::stream(h)));
    return PM_OK;
  };
  float low = 0.f, high = 0.5f;
  const float first = (float)(1.5 * percentile);
  unsigned n_dark = 0;
  if (int rc = count_at(first, &n_dark)) return rc;
  if ((int)n_dark < n_desired) {
    low = first;
  } else if ((int)n_dark > n_desired) {
    high = first;
  } else {
    *threshold = first;
    return PM_OK;
  }
  for (int iter = 0; iter < 8; ++iter) {
    const float thr = (high + low) / 2.0f;
    if (int rc = count_at(thr, &n_dark)) return rc;
    if ((int)n_dark < n_desired) {
      low = thr;
    } else if ((int)n_dark > n_desired) {
      high = thr;
    } else {
      *threshold = thr;
      return PM_OK;
    }
  }
  *threshold = (high + low) / 2.0f;
  return PM_OK;
}

// ---- stereo-ready enhancement ---------------------------------------------------------------------
namespace {

// cv::getGaussianKernel(n, sigma, CV_32F), uploaded once per (n, sigma)
int ensure_taps(pm_handle* h, int ksize, double sigma) {
  ImagingState* st = state_of(h);
  if (st->enh_ksize == ksize && st->enh_sigma == sigma && st->enh_taps) return PM_OK;
  bool gone = false;
  PM_HIP(h, st->enh_taps.reserve(sizeof(float) * (size_t)ksize, pm_internal::stream(h), &gone));
  if (gone) st->enh_ksize = 0;  // the cached taps went with the old buffer
  std::vector<float> k((size_t)ksize);
  const double scale2x = -0.5 / (sigma * sigma);
  double sum = 0;
  for (int i = 0; i < ksize; ++i) {
    const double x = i - (ksize - 1) * 0.5;
    k[(size_t)i] = (float)std::exp(scale2x * x * x);
    sum += k[(size_t)i];
  }
  sum = 1. / sum;
  for (int i = 0; i < ksize; ++i) k[(size_t)i] = (float)(k[(size_t)i] * sum);
  PM_HIP(h, hipStreamSynchronize(pm_internal::stream(h)));  // the previous taps may still be in use
  PM_HIP(h, hipMemcpy(st->enh_taps, k.data(), sizeof(float) * (size_t)ksize, hipMemcpyHostToDevice));
  st->enh_ksize = ksize;
  st->enh_sigma = sigma;
  return PM_OK;
}

int ensure_enh_scratch(pm_handle* h, size_t values) {
  PM_HIP(h, state_of(h)->enh_tmp.reserve(sizeof(float) * values, pm_internal::stream(h)));
  PM_HIP(h, state_of(h)->enh_q.reserve(sizeof(float) * values, pm_internal::stream(h)));
  return PM_OK;
}

// separable Gaussian, replicate border, of `count` <= kBlurBatch images of one size in one launch per pass; divide:
// dst = orig / (2 * blur) (the illuminant normalisation)
template <bool SRC_U8>
int run_gaussian_batch(pm_handle* h, const void* const* d_src, float* const* d_dst, int count, int rows, int cols, int ch,
                       int ksize, double sigma, bool divide) {
  if (ksize < 1 || (ksize % 2) == 0 || !(sigma > 0)) {
    set_err(h, "gaussian: ksize %d must be odd and sigma %g positive", ksize, sigma);
    return PM_ERR_INVALID_ARG;
  }
  if (count < 1 || count > kBlurBatch) {
    set_err(h, "gaussian: %d images in one batch (1 .. %d)", count, kBlurBatch);
    return PM_ERR_INVALID_ARG;
  }
  const size_t values = (size_t)rows * cols * ch;
  if (int rc = ensure_enh_scratch(h, values * (size_t)count)) return rc;
  if (int rc = ensure_taps(h, ksize, sigma)) return rc;
  const size_t row_lds = sizeof(float) * ((size_t)(blur_skew(kBlurRowPx + ksize - 1) + 1) * ch + ksize);
  if (row_lds > 64 * 1024) {
    set_err(h, "gaussian: kernel of %d taps x %d channels exceeds the row tile", ksize, ch);
    return PM_ERR_SIZE;
  }
  BlurBatch bb{};
  for (int i = 0; i < count; ++i) {
    bb.src[i] = d_src[i];
    bb.dst[i] = d_dst[i];
  }
  bb.tmp = state_of(h)->enh_tmp;
  bb.tmp_stride = values;
  const dim3 rgrid((unsigned)((cols + kBlurRowPx - 1) / kBlurRowPx), (unsigned)rows, (unsigned)count);
  const float* taps = state_of(h)->enh_taps;
  hipStream_t stream = pm_internal::stream(h);
  switch (ch) {
    case 1: hipLaunchKernelGGL((k_blur_rows<SRC_U8, 1>), rgrid, dim3(kBlurRowThreads), row_lds, stream, bb, rows, cols, ksize, taps); break;
    case 2: hipLaunchKernelGGL((k_blur_rows<SRC_U8, 2>), rgrid, dim3(kBlurRowThreads), row_lds, stream, bb, rows, cols, ksize, taps); break;
    case 3: hipLaunchKernelGGL((k_blur_rows<SRC_U8, 3>), rgrid, dim3(kBlurRowThreads), row_lds, stream, bb, rows, cols, ksize, taps); break;
    default: hipLaunchKernelGGL((k_blur_rows<SRC_U8, 4>), rgrid, dim3(kBlurRowThreads), row_lds, stream, bb, rows, cols, ksize, taps); break;
  }
  // column tile: W columns x T rows of outputs with T = (threads / (W / 2)) * 4 -- one group of four rows per thread --
  // and ((T + 2c + 3) x (W + 2) + c + 1) floats of LDS; the widest tile that fits 48 KB (wider = better coalesced fill)
  const int c = ksize / 2;
  int W = 0, T = 0, NT = 256;
  {
    static const std::array<int, 3> forced = [] {  // PM_BLUR_COL = "W,T,threads" (experiments), read once
      int w = 0, t = 0, n = 0;
      const char* e = pm::tune_env("PM_BLUR_COL");
      if (e && sscanf(e, "%d,%d,%d", &w, &t, &n) == 3) return std::array<int, 3>{w, t, n};
      return std::array<int, 3>{0, 0, 0};
    }();
    auto lds_of = [&](int w, int t) { return sizeof(float) * ((size_t)(t + 2 * c + 3) * (w + 2) + c + 1); };
    if (forced[0]) {
      W = forced[0];
      T = forced[1];
      NT = forced[2];
    } else {
      for (int w : {32, 16, 8}) {
        const int t = (256 / (w / 2)) * 4;
        if (lds_of(w, t) <= 48 * 1024) {
          W = w;
          T = t;
          break;
        }
      }
    }
    if (!W || lds_of(W, T) > 64 * 1024) {
      set_err(h, "gaussian: kernel of %d taps exceeds the column tile", ksize);
      return PM_ERR_SIZE;
    }
  }
  const int width = cols * ch;
  const size_t col_lds = sizeof(float) * ((size_t)(T + 2 * c + 3) * (W + 2) + c + 1);
  const dim3 cgrid((unsigned)((width + W - 1) / W), (unsigned)((rows + T - 1) / T), (unsigned)count);
  if (divide)
    hipLaunchKernelGGL((k_blur_cols<true, SRC_U8>), cgrid, dim3(NT), col_lds, stream, bb, rows, width, ksize, taps, W, T);
  else
    hipLaunchKernelGGL((k_blur_cols<false, SRC_U8>), cgrid, dim3(NT), col_lds, stream, bb, rows, width, ksize, taps, W, T);
  return launch_check(h, "gaussian");
}
template <bool SRC_U8>
int run_gaussian(pm_handle* h, const void* d_src, int rows, int cols, int ch, int ksize, double sigma, bool divide,
                 float* d_dst) {
  return run_gaussian_batch<SRC_U8>(h, &d_src, &d_dst, 1, rows, cols, ch, ksize, sigma, divide);
}

// imaging::Normalize on d_q -> J and / or gray8
int run_normalize(pm_handle* h, const float* d_q, int rows, int cols, float* d_J, uint8_t* d_gray8) {
  if (rows < 8 || cols < 8) {
    set_err(h, "normalize: the image must be at least 8x8 (its 1/8 resize would be empty)");
    return PM_ERR_INVALID_ARG;
  }
  const unsigned init[2] = {kValueMinInit, kValueMaxInit};
  PM_HIP(h, hipMemcpyAsync(state_of(h)->img_scalars + 2, init, sizeof(init), hipMemcpyHostToDevice, pm_internal::stream(h)));
  const size_t small = (size_t)(rows / 8) * (cols / 8);
  hipLaunchKernelGGL(k_value_minmax, reduce_grid(small), dim3(256), 0, pm_internal::stream(h), d_q, rows, cols, state_of(h)->img_scalars + 2);
  const size_t n = (size_t)rows * cols;
  hipLaunchKernelGGL(k_normalize_gray, stream_grid(n), dim3(256), 0, pm_internal::stream(h), d_q, n,
                     (const unsigned*)(state_of(h)->img_scalars + 2), d_J, d_gray8);
  return launch_check(h, "normalize");
}

}  // namespace

int pm_gaussian_blur(pm_handle* h, const float* d_src, int rows, int cols, int channels, int ksize, double sigma,
                     float* d_dst) {
  if (int rc = imaging_begin(h, "pm_gaussian_blur", d_src, d_dst, rows, cols)) return rc;
  if (channels < 1 || channels > 4) {
    set_err(h, "pm_gaussian_blur: %d channels", channels);
    return PM_ERR_INVALID_ARG;
  }
  return run_gaussian<false>(h, d_src, rows, cols, channels, ksize, sigma, false, d_dst);
}

int pm_normalize(pm_handle* h, const float* d_bgr, int rows, int cols, float* d_out) {
  if (int rc = imaging_begin(h, "pm_normalize", d_bgr, d_out, rows, cols)) return rc;
  return run_normalize(h, d_bgr, rows, cols, d_out, nullptr);
}

int pm_stereo_ready(pm_handle* h, const uint8_t* d_bgr8, int rows, int cols, float* d_J, uint8_t* d_gray8) {
  if (int rc = imaging_begin(h, "pm_stereo_ready", d_bgr8, d_bgr8, rows, cols)) return rc;
  if (!d_J && !d_gray8) {
    set_err(h, "pm_stereo_ready: no output requested");
    return PM_ERR_INVALID_ARG;
  }
  // NormalizeColorIlluminant (normalization.cpp:178-185): ksize = NextOddInt(cols / 3), sigma = (float)ksize / 4
  const int third = cols / 3;
  const int ksize = third + (1 - third % 2);
  const double sigma = (double)((float)ksize / 4.0f);
  if (int rc = ensure_enh_scratch(h, (size_t)rows * cols * 3)) return rc;
  if (int rc = run_gaussian<true>(h, d_bgr8, rows, cols, 3, ksize, sigma, true, state_of(h)->enh_q)) return rc;
  // enhance_test.cpp:69 applies Normalize to NormalizeColorIlluminant's result, which already ends with a
  // Normalize (normalization.cpp:184): two value stretches.  The row-pass scratch is free again: it takes the first.
  if (int rc = run_normalize(h, state_of(h)->enh_q, rows, cols, state_of(h)->enh_tmp, nullptr)) return rc;
  return run_normalize(h, state_of(h)->enh_tmp, rows, cols, d_J, d_gray8);
}

// Match() on BGR inputs with the stereo-ready enhancement folded into the load path (BASELINE configs[4]): per image the
// two Gaussian passes (illuminant estimate) and the two tiny min / max passes of the value stretches; everything per
// pixel happens inside k_prep_bgr.  Results equal pm_stereo_ready x 2 followed by pm_match_device bit for bit.
int pm_match_bgr_device(pm_handle* h, int n, const uint8_t* d_left_bgr8, const uint8_t* d_right_bgr8, int rows, int cols,
                        const float* d_seed_l, const float* d_seed_r, float* d_disp_l, float* d_disp_r) {
  if (int rc = imaging_begin(h, "pm_match_bgr_device", d_left_bgr8, d_right_bgr8, rows, cols)) return rc;
  if (n < 1 || rows < 8 || cols < 8) {
    set_err(h, "pm_match_bgr_device: n >= 1 pairs of at least 8x8 pixels");
    return PM_ERR_INVALID_ARG;
  }
  ImagingState& st = *state_of(h);
  const size_t ipx = (size_t)rows * cols, values = ipx * 3;
  PM_HIP(h, st.bgr_blur.reserve(sizeof(float) * values * 2 * (size_t)n, pm_internal::stream(h)));
  PM_HIP(h, st.bgr_mm.reserve(sizeof(unsigned) * 8 * (size_t)n, pm_internal::stream(h)));
  // NormalizeColorIlluminant (normalization.cpp:178-185): ksize = NextOddInt(cols / 3), sigma = (float)ksize / 4
  const int third = cols / 3;
  const int ksize = third + (1 - third % 2);
  const double sigma = (double)((float)ksize / 4.0f);
  std::vector<unsigned> init((size_t)n * 8);
  for (size_t i = 0; i < init.size(); i += 2) {
    init[i] = kValueMinInit;
    init[i + 1] = kValueMaxInit;
  }
  PM_HIP(h, hipMemcpyAsync(st.bgr_mm, init.data(), sizeof(unsigned) * init.size(), hipMemcpyHostToDevice, pm_internal::stream(h)));
  float* blur_l = st.bgr_blur;
  float* blur_r = st.bgr_blur + values * (size_t)n;
  const size_t small = (size_t)(rows / 8) * (cols / 8);
  // image z = b * 2 + i (pair b, left / right); up to kBlurBatch images per launch of each pass
  for (int z0 = 0; z0 < 2 * n; z0 += kBlurBatch) {
    const int count = 2 * n - z0 < kBlurBatch ? 2 * n - z0 : kBlurBatch;
    const void* srcs[kBlurBatch];
    float* dsts[kBlurBatch];
    BlurBatch bb{};
    for (int k = 0; k < count; ++k) {
      const int b = (z0 + k) >> 1, i = (z0 + k) & 1;
      srcs[k] = (i == 0 ? d_left_bgr8 : d_right_bgr8) + (size_t)b * values;
      dsts[k] = (i == 0 ? blur_l : blur_r) + (size_t)b * values;
      bb.src[k] = srcs[k];
      bb.dst[k] = dsts[k];
    }
    if (int rc = run_gaussian_batch<true>(h, srcs, dsts, count, rows, cols, 3, ksize, sigma, false)) return rc;
    dim3 mgrid = reduce_grid(small);
    mgrid.y = (unsigned)count;
    unsigned* mm = st.bgr_mm + (size_t)z0 * 4;
    hipLaunchKernelGGL((k_value_minmax_fused<1>), mgrid, dim3(256), 0, pm_internal::stream(h), bb, rows, cols, mm);
    hipLaunchKernelGGL((k_value_minmax_fused<2>), mgrid, dim3(256), 0, pm_internal::stream(h), bb, rows, cols, mm);
  }
  if (int rc = launch_check(h, "value min / max")) return rc;
  BgrSource src;
  src.left = d_left_bgr8;
  src.right = d_right_bgr8;
  src.blur_l = blur_l;
  src.blur_r = blur_r;
  src.mm = st.bgr_mm;
  return pm_internal::match_bgr(h, n, src, rows, cols, d_seed_l, d_seed_r, d_disp_l, d_disp_r);
}

int pm_normalize_color_illuminant(pm_handle* h, const float* d_bgr, int rows, int cols, float* d_out) {
  if (int rc = imaging_begin(h, "pm_normalize_color_illuminant", d_bgr, d_out, rows, cols)) return rc;
  const int third = cols / 3;
  const int ksize = third + (1 - third % 2);
  const double sigma = (double)((float)ksize / 4.0f);
  if (int rc = ensure_enh_scratch(h, (size_t)rows * cols * 3)) return rc;
  if (int rc = run_gaussian<false>(h, d_bgr, rows, cols, 3, ksize, sigma, true, state_of(h)->enh_q)) return rc;
  return run_normalize(h, state_of(h)->enh_q, rows, cols, d_out, nullptr);
}

// ---- fast guided filter with a one-channel guide, and the pixel gather (pm_guided.hpp) -----------------------------
namespace {

int run_guided_filter(pm_handle* h, const char* what, const float* d_guide, const float* d_src, int rows, int cols,
                      int channels, int r, double eps, int s, float scale, float* d_dst) {
  if (int rc = imaging_begin(h, what, d_guide, d_src, rows, cols)) return rc;
  if (!d_dst) {
    set_err(h, "%s: null output", what);
    return PM_ERR_INVALID_ARG;
  }
  if (channels < 1 || channels > 4) {
    set_err(h, "%s: %d channels (1 .. 4)", what, channels);
    return PM_ERR_INVALID_ARG;
  }
  if (s < 1 || r < 0 || rows / s < 1 || cols / s < 1) {
    set_err(h, "%s: r = %d must be >= 0, s = %d >= 1, and the %dx%d image at least s x s", what, r, s, cols, rows);
    return PM_ERR_INVALID_ARG;
  }
  if (!(eps >= 0) || !std::isfinite(eps)) {
    set_err(h, "%s: eps = %g must be finite and >= 0", what, eps);
    return PM_ERR_INVALID_ARG;
  }
  GfShape g{};
  g.rows = rows;
  g.cols = cols;
  g.crows = rows / s;
  g.ccols = cols / s;
  g.channels = channels;
  g.k = 2 * (r / s) + 1;  // fast_guided_filter.cpp:211-214
  g.inv_y = 1.0 / ((double)g.crows / rows);
  g.inv_x = 1.0 / ((double)g.ccols / cols);
  g.up_y = 1.0 / ((double)rows / g.crows);
  g.up_x = 1.0 / ((double)cols / g.ccols);
  const size_t row_lds = sizeof(float) * (size_t)g.ccols;
  if (row_lds > 64 * 1024) {
    set_err(h, "%s: a coarse row of %d pixels exceeds the row tile", what, g.ccols);
    return PM_ERR_SIZE;
  }
  ImagingState* st = state_of(h);
  const size_t cpx = (size_t)g.crows * g.ccols;
  const int planes1 = 2 + 2 * channels, planes2 = 2 * channels;
  const size_t sum_bytes = sizeof(double) * cpx * planes1, ab_bytes = sizeof(float) * cpx * planes2;
  hipStream_t stream = pm_internal::stream(h);
  PM_HIP(h, st->gf_buf.reserve(sum_bytes + 2 * ab_bytes, stream));
  double* rowsum = (double*)st->gf_buf.get();
  float* ab = (float*)(st->gf_buf + sum_bytes);
  float* mean = (float*)(st->gf_buf + sum_bytes + ab_bytes);
  const dim3 cgrid((unsigned)((cpx + 127) / 128), (unsigned)channels);
  hipLaunchKernelGGL((k_gf_box_rows<true>), dim3((unsigned)g.crows, (unsigned)planes1), dim3(256), row_lds, stream, d_guide,
                     d_src, (const float*)nullptr, g, rowsum);
  hipLaunchKernelGGL(k_gf_box_cols_ab, cgrid, dim3(128), 0, stream, (const double*)rowsum, g, (float)eps, ab);
  hipLaunchKernelGGL((k_gf_box_rows<false>), dim3((unsigned)g.crows, (unsigned)planes2), dim3(256), row_lds, stream,
                     (const float*)nullptr, (const float*)nullptr, (const float*)ab, g, rowsum);
  hipLaunchKernelGGL(k_gf_box_cols_mean, cgrid, dim3(128), 0, stream, (const double*)rowsum, g, mean);
  const size_t n = (size_t)rows * cols;
  const int vec = aligned16(d_guide) && aligned16(d_dst);
  const dim3 agrid = stream_grid(n / 4 + 1);
  switch (channels) {
    case 1: hipLaunchKernelGGL((k_gf_apply<1>), agrid, dim3(256), 0, stream, d_guide, (const float*)mean, g, scale, d_dst, vec); break;
    case 2: hipLaunchKernelGGL((k_gf_apply<2>), agrid, dim3(256), 0, stream, d_guide, (const float*)mean, g, scale, d_dst, vec); break;
    case 3: hipLaunchKernelGGL((k_gf_apply<3>), agrid, dim3(256), 0, stream, d_guide, (const float*)mean, g, scale, d_dst, vec); break;
    default: hipLaunchKernelGGL((k_gf_apply<4>), agrid, dim3(256), 0, stream, d_guide, (const float*)mean, g, scale, d_dst, vec); break;
  }
  return launch_check(h, "guided filter");
}

}  // namespace

int pm_fast_guided_filter(pm_handle* h, const float* d_guide, const float* d_src, int rows, int cols, int channels, int r,
                          double eps, int s, float scale, float* d_dst) {
  return run_guided_filter(h, "pm_fast_guided_filter", d_guide, d_src, rows, cols, channels, r, eps, s, scale, d_dst);
}

int pm_estimate_illuminant_range_guided(pm_handle* h, const float* d_bgr, const float* d_range, int rows, int cols, int r,
                                        double eps, int s, float* d_illuminant) {
  // Akkaynak et al. multiply by a factor of 2 to get the illuminant map (illuminant.cpp:31-33)
  return run_guided_filter(h, "pm_estimate_illuminant_range_guided", d_range, d_bgr, rows, cols, 3, r, eps, s, 2.0f,
                           d_illuminant);
}

int pm_gather_pixels(pm_handle* h, const float* d_img, int rows, int cols, int channels, const int32_t* d_xy,
                     const int32_t* xy, int n, float* host_out) {
  if (int rc = imaging_begin(h, "pm_gather_pixels", d_img, d_img, rows, cols)) return rc;
  if (channels < 1 || channels > 4 || n < 0 || (d_xy != nullptr) == (xy != nullptr) || (n > 0 && !host_out)) {
    set_err(h, "pm_gather_pixels: 1 .. 4 channels, n >= 0, exactly one of d_xy / xy, and an output for n > 0");
    return PM_ERR_INVALID_ARG;
  }
  if (xy)
    for (int i = 0; i < n; ++i)
      if (xy[2 * i] < 0 || xy[2 * i] >= cols || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= rows) {
        set_err(h, "pm_gather_pixels: entry %d (x = %d, y = %d) lies outside the %dx%d image", i, xy[2 * i], xy[2 * i + 1],
                cols, rows);
        return PM_ERR_INVALID_ARG;
      }
  if (n == 0) return PM_OK;
  ImagingState* st = state_of(h);
  const size_t head = 16, val_bytes = sizeof(float) * (size_t)n * channels, xy_bytes = sizeof(int32_t) * 2 * (size_t)n;
  hipStream_t stream = pm_internal::stream(h);
  PM_HIP(h, st->gat_buf.reserve(head + val_bytes + xy_bytes, stream));
  unsigned* d_bad = (unsigned*)st->gat_buf.get();
  float* d_val = (float*)(st->gat_buf + head);
  const int32_t* d_coords = d_xy;
  if (xy) {
    int32_t* d_copy = (int32_t*)(st->gat_buf + head + val_bytes);
    PM_HIP(h, hipMemcpyAsync(d_copy, xy, xy_bytes, hipMemcpyHostToDevice, stream));
    d_coords = d_copy;
  }
  PM_HIP(h, hipMemsetAsync(st->gat_buf, 0, head + val_bytes, stream));
  hipLaunchKernelGGL(k_gather_pixels, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_img, rows, cols, channels,
                     d_coords, n, d_val, d_bad);
  if (int rc = launch_check(h, "gather_pixels")) return rc;
  // flag and values arrive together; host_out is written only when every entry was inside the image
  std::vector<unsigned char> landed(head + val_bytes);
  PM_HIP(h, hipMemcpyAsync(landed.data(), st->gat_buf, head + val_bytes, hipMemcpyDeviceToHost, stream));
  PM_HIP(h, hipStreamSynchronize(stream));
  unsigned bad = 0;
  std::memcpy(&bad, landed.data(), sizeof(bad));
  if (bad) {
    set_err(h, "pm_gather_pixels: a coordinate of d_xy lies outside the %dx%d image", cols, rows);
    return PM_ERR_INVALID_ARG;
  }
  std::memcpy(host_out, landed.data() + head, val_bytes);
  return PM_OK;
}

// ---- undistortion + rectification in front of Match() (pm_rectify.hpp) ----------------------------------------------
namespace {

// the checks of a view that every entry point shares; `which` names it in the error text
int check_view(pm_handle* h, const char* what, const char* which, const pm_rectify_view* v) {
  if (!v) {
    set_err(h, "%s: null %s", what, which);
    return PM_ERR_INVALID_ARG;
  }
  const double* e = reinterpret_cast<const double*>(v);
  static_assert(sizeof(pm_rectify_view) == 22 * sizeof(double), "pm_rectify_view is 22 doubles");
  for (int i = 0; i < 22; ++i)
    if (!std::isfinite(e[i])) {
      set_err(h, "%s: entry %d of %s is not finite", what, i, which);
      return PM_ERR_INVALID_ARG;
    }
  if (v->fx_new == 0.0 || v->fy_new == 0.0) {
    set_err(h, "%s: fx_new / fy_new of %s must not be 0", what, which);
    return PM_ERR_INVALID_ARG;
  }
  return PM_OK;
}

// channels: bytes per source pixel (1 gray, 3 interleaved BGR).  *src_step == 0 means packed and becomes the row's
// channels * src_cols bytes.
int check_rectify_shape(pm_handle* h, const char* what, int channels, int n, int src_rows, int src_cols, size_t* src_step,
                        int rows, int cols, int border_value) {
  if (n < 1 || src_rows < 1 || src_cols < 1 || rows < 1 || cols < 1) {
    set_err(h, "%s: %d images of %dx%d from %dx%d: every count and size must be >= 1", what, n, cols, rows, src_cols, src_rows);
    return PM_ERR_INVALID_ARG;
  }
  const size_t row = (size_t)channels * src_cols;
  if (*src_step == 0) *src_step = row;
  if (*src_step < row) {
    set_err(h, "%s: src_step %zu is smaller than a row of %d %s", what, *src_step, src_cols,
            channels == 3 ? "BGR pixels" : "bytes");
    return PM_ERR_INVALID_ARG;
  }
  if (border_value < 0 || border_value > 255) {
    set_err(h, "%s: border_value %d outside 0 .. 255", what, border_value);
    return PM_ERR_INVALID_ARG;
  }
  if (n > 65535 || (rows + kRectifyBlockY - 1) / kRectifyBlockY > 65535) {
    set_err(h, "%s: %d images of %d rows exceed the launch grid", what, n, rows);
    return PM_ERR_SIZE;
  }
  return PM_OK;
}

// arguments already checked; n: the images of the launch (grid z)
template <RectifyKind KIND>
void launch_rectify(const RectifyArgs& a, int n, hipStream_t stream) {
  const int px = kRectifyBlockX * 4;
  const dim3 grid((unsigned)((a.cols + px - 1) / px), (unsigned)((a.rows + kRectifyBlockY - 1) / kRectifyBlockY), (unsigned)n);
  hipLaunchKernelGGL((k_rectify<KIND>), grid, dim3(kRectifyBlockX, kRectifyBlockY), 0, stream, a);
}
// channels 1: gray (d_dstf null); 3: BGR, with the float image where d_dstf is given
void launch_rectify(int channels, const pm_rectify_view& view, const uint8_t* d_src, int n, int src_rows, int src_cols,
                    size_t src_step, int rows, int cols, int border_value, uint8_t* d_dst, float* d_dstf, uint8_t* d_valid,
                    hipStream_t stream) {
  const RectifyArgs a = {view, d_src, src_rows, src_cols, src_step, rows, cols, border_value, d_dst, d_dstf, d_valid, nullptr};
  if (channels == 1)
    launch_rectify<RectifyKind::Gray>(a, n, stream);
  else if (d_dstf)
    launch_rectify<RectifyKind::BgrFloat>(a, n, stream);
  else
    launch_rectify<RectifyKind::Bgr>(a, n, stream);
}

// What pm_match_raw_device (channels 1) and pm_match_raw_bgr_device (channels 3) share: every check, then the two
// rectifications into the handle's scratch -- or into d_keep_l / d_keep_r where the caller keeps a rectified image, which
// is then matched from there -- and the Match() of `match` on the result.
typedef int (*MatchFn)(pm_handle*, int, const uint8_t*, const uint8_t*, int, int, const float*, const float*, float*, float*);
int match_raw(pm_handle* h, const char* what, int channels, MatchFn match, int n, const pm_rectify_view* left,
              const pm_rectify_view* right, const uint8_t* d_left_raw, const uint8_t* d_right_raw, int src_rows, int src_cols,
              size_t src_step, int rows, int cols, const float* d_seed_l, const float* d_seed_r, float* d_disp_l,
              float* d_disp_r, uint8_t* d_keep_l, uint8_t* d_keep_r) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (!d_left_raw || !d_right_raw || !d_disp_l) {
    set_err(h, "%s: null image or output pointer", what);
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_view(h, what, "left view", left)) return rc;
  if (int rc = check_view(h, what, "right view", right)) return rc;
  if (int rc = check_rectify_shape(h, what, channels, n, src_rows, src_cols, &src_step, rows, cols, 0)) return rc;
  int max_rows = 0, max_cols = 0;
  pm_internal::plan_size(h, &max_rows, &max_cols);
  if (rows < 8 || cols < 8) {
    set_err(h, "%s: rectified image %dx%d too small (min 8x8)", what, cols, rows);
    return PM_ERR_INVALID_ARG;
  }
  if (rows > max_rows || cols > max_cols) {
    set_err(h, "%s: rectified size %dx%d exceeds plan %dx%d", what, cols, rows, max_cols, max_rows);
    return PM_ERR_SIZE;
  }
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  ImagingState* st = state_of(h);
  if (!st) {
    set_err(h, "%s: out of host memory", what);
    return PM_ERR_NOMEM;
  }
  const size_t side = (size_t)n * rows * cols * channels;
  const int own = (d_keep_l ? 0 : 1) + (d_keep_r ? 0 : 1);
  hipStream_t stream = pm_internal::stream(h);
  if (own) PM_HIP(h, st->rect_buf.reserve(own * side, stream));
  uint8_t* rect_l = d_keep_l ? d_keep_l : st->rect_buf.get();
  uint8_t* rect_r = d_keep_r ? d_keep_r : st->rect_buf.get() + (own - 1) * side;
  launch_rectify(channels, *left, d_left_raw, n, src_rows, src_cols, src_step, rows, cols, 0, rect_l, nullptr, nullptr, stream);
  launch_rectify(channels, *right, d_right_raw, n, src_rows, src_cols, src_step, rows, cols, 0, rect_r, nullptr, nullptr, stream);
  if (int rc = launch_check(h, channels == 3 ? "rectify bgr" : "rectify")) return rc;
  return match(h, n, rect_l, rect_r, rows, cols, d_seed_l, d_seed_r, d_disp_l, d_disp_r);
}

}  // namespace

int pm_rectify_u8(pm_handle* h, const pm_rectify_view* view, const uint8_t* d_src, int n, int src_rows, int src_cols,
                  size_t src_step, int rows, int cols, int border_value, uint8_t* d_dst, uint8_t* d_valid, void* stream) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (!d_src || !d_dst) {
    set_err(h, "pm_rectify_u8: null image pointer");
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_view(h, "pm_rectify_u8", "view", view)) return rc;
  if (int rc = check_rectify_shape(h, "pm_rectify_u8", 1, n, src_rows, src_cols, &src_step, rows, cols, border_value)) return rc;
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  launch_rectify(1, *view, d_src, n, src_rows, src_cols, src_step, rows, cols, border_value, d_dst, nullptr, d_valid,
                 stream ? (hipStream_t)stream : pm_internal::stream(h));
  return launch_check(h, "rectify");
}

int pm_rectify_map(pm_handle* h, const pm_rectify_view* view, int rows, int cols, int32_t* d_xy) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (!d_xy) {
    set_err(h, "pm_rectify_map: null output");
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_view(h, "pm_rectify_map", "view", view)) return rc;
  size_t step = 0;
  if (int rc = check_rectify_shape(h, "pm_rectify_map", 1, 1, 1, 1, &step, rows, cols, 0)) return rc;
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  const RectifyArgs a = {*view, nullptr, 0, 0, 0, rows, cols, 0, nullptr, nullptr, nullptr, d_xy};
  launch_rectify<RectifyKind::Map>(a, 1, pm_internal::stream(h));
  return launch_check(h, "rectify map");
}

int pm_match_raw_device(pm_handle* h, int n, const pm_rectify_view* left, const pm_rectify_view* right,
                        const uint8_t* d_left_raw, const uint8_t* d_right_raw, int src_rows, int src_cols, size_t src_step,
                        int rows, int cols, const float* d_seed_l, const float* d_seed_r, float* d_disp_l, float* d_disp_r) {
  return match_raw(h, "pm_match_raw_device", 1, pm_match_device, n, left, right, d_left_raw, d_right_raw, src_rows, src_cols,
                   src_step, rows, cols, d_seed_l, d_seed_r, d_disp_l, d_disp_r, nullptr, nullptr);
}

int pm_rectify_bgr8(pm_handle* h, const pm_rectify_view* view, const uint8_t* d_src_bgr8, int n, int src_rows, int src_cols,
                    size_t src_step, int rows, int cols, int border_value, uint8_t* d_dst_bgr8, float* d_dst_bgr32f,
                    uint8_t* d_valid, void* stream) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (!d_src_bgr8 || (!d_dst_bgr8 && !d_dst_bgr32f)) {
    set_err(h, "pm_rectify_bgr8: null source, or neither the 8-bit nor the float image requested");
    return PM_ERR_INVALID_ARG;
  }
  if (int rc = check_view(h, "pm_rectify_bgr8", "view", view)) return rc;
  if (int rc = check_rectify_shape(h, "pm_rectify_bgr8", 3, n, src_rows, src_cols, &src_step, rows, cols, border_value)) return rc;
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  launch_rectify(3, *view, d_src_bgr8, n, src_rows, src_cols, src_step, rows, cols, border_value, d_dst_bgr8, d_dst_bgr32f,
                 d_valid, stream ? (hipStream_t)stream : pm_internal::stream(h));
  return launch_check(h, "rectify bgr");
}

int pm_match_raw_bgr_device(pm_handle* h, int n, const pm_rectify_view* left, const pm_rectify_view* right,
                            const uint8_t* d_left_raw_bgr8, const uint8_t* d_right_raw_bgr8, int src_rows, int src_cols,
                            size_t src_step, int rows, int cols, const float* d_seed_l, const float* d_seed_r,
                            float* d_disp_l, float* d_disp_r, uint8_t* d_left_rect_bgr8, uint8_t* d_right_rect_bgr8) {
  return match_raw(h, "pm_match_raw_bgr_device", 3, pm_match_bgr_device, n, left, right, d_left_raw_bgr8, d_right_raw_bgr8,
                   src_rows, src_cols, src_step, rows, cols, d_seed_l, d_seed_r, d_disp_l, d_disp_r, d_left_rect_bgr8,
                   d_right_rect_bgr8);
}

// Host only: Bouguet's construction (see pm/imaging.h).
namespace {

struct Mat3 {
  double m[9];
};
Mat3 mul(const Mat3& a, const Mat3& b) {
  Mat3 c{};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c.m[3 * i + j] = (a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j]) + a.m[3 * i + 2] * b.m[6 + j];
  return c;
}
Mat3 transpose(const Mat3& a) {
  Mat3 t{};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) t.m[3 * i + j] = a.m[3 * j + i];
  return t;
}
// Rodrigues: the rotation by |w| about w; |w| == 0 gives I exactly
Mat3 rotation_of(const double w[3]) {
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  Mat3 r{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
  if (th == 0.0) return r;
  const double k[3] = {w[0] / th, w[1] / th, w[2] / th};
  const double c = std::cos(th), s = std::sin(th), v = 1.0 - c;
  r.m[0] = c + v * k[0] * k[0];
  r.m[1] = v * k[0] * k[1] - s * k[2];
  r.m[2] = v * k[0] * k[2] + s * k[1];
  r.m[3] = v * k[1] * k[0] + s * k[2];
  r.m[4] = c + v * k[1] * k[1];
  r.m[5] = v * k[1] * k[2] - s * k[0];
  r.m[6] = v * k[2] * k[0] - s * k[1];
  r.m[7] = v * k[2] * k[1] + s * k[0];
  r.m[8] = c + v * k[2] * k[2];
  return r;
}

}  // namespace

int pm_stereo_rectify(const pm_camera* c1, const pm_camera* c2, const double R[9], const double T[3], pm_rectify_view* v1,
                      pm_rectify_view* v2, double* baseline) {
  if (!c1 || !c2 || !R || !T || !v1 || !v2 || !baseline) return PM_ERR_INVALID_ARG;
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(R[i]) || !std::isfinite(reinterpret_cast<const double*>(c1)[i]) ||
        !std::isfinite(reinterpret_cast<const double*>(c2)[i]))
      return PM_ERR_INVALID_ARG;
  const double len = std::sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2]);
  if (!std::isfinite(len) || len == 0.0) return PM_ERR_INVALID_ARG;
  // R = exp([om]x): om = axis * angle, from the skew part (sine) and the trace (cosine)
  const double sk[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
  const double s = std::sqrt(sk[0] * sk[0] + sk[1] * sk[1] + sk[2] * sk[2]);
  const double c = 0.5 * ((R[0] + R[4] + R[8]) - 1.0);
  if (c < -0.99) return PM_ERR_INVALID_ARG;  // cameras that look in opposite directions
  double half[3] = {0, 0, 0};                // -om / 2
  if (s > 0.0) {
    const double scale = -0.5 * std::atan2(s, c) / s;
    for (int i = 0; i < 3; ++i) half[i] = sk[i] * scale;
  }
  const Mat3 r_r = rotation_of(half);  // R^(-1/2): turns camera 2; its transpose turns camera 1
  const double t[3] = {(r_r.m[0] * T[0] + r_r.m[1] * T[1]) + r_r.m[2] * T[2], (r_r.m[3] * T[0] + r_r.m[4] * T[1]) + r_r.m[5] * T[2],
                       (r_r.m[6] * T[0] + r_r.m[7] * T[1]) + r_r.m[8] * T[2]};
  if (!(t[0] < 0.0)) return PM_ERR_INVALID_ARG;  // camera 1 is not the left one
  // the rotation that takes t onto -x: axis t x (-1, 0, 0) = (0, -t2, t1), angle acos(-t0 / |t|)
  double ww[3] = {0.0, -t[2], t[1]};
  const double nw = std::sqrt(ww[1] * ww[1] + ww[2] * ww[2]);
  if (nw > 0.0) {
    const double angle = std::atan2(nw, -t[0]);
    ww[1] = ww[1] * (angle / nw);
    ww[2] = ww[2] * (angle / nw);
  }
  const Mat3 w_r = rotation_of(ww);
  const Mat3 r1 = mul(w_r, transpose(r_r)), r2 = mul(w_r, r_r);
  const double f = c1->fy < c2->fy ? c1->fy : c2->fy;
  pm_rectify_view* out[2] = {v1, v2};
  const pm_camera* cam[2] = {c1, c2};
  const Mat3* rot[2] = {&r1, &r2};
  for (int i = 0; i < 2; ++i) {
    out[i]->cam = *cam[i];
    for (int k = 0; k < 9; ++k) out[i]->R[k] = rot[i]->m[k];
    out[i]->fx_new = out[i]->fy_new = f;
    out[i]->cx_new = 0.5 * (c1->cx + c2->cx);
    out[i]->cy_new = 0.5 * (c1->cy + c2->cy);
  }
  *baseline = len;
  return PM_OK;
}

int pm_device_malloc(pm_handle* h, size_t bytes, void** d_ptr) {
  if (!h || !d_ptr) return PM_ERR_INVALID_ARG;
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  *d_ptr = nullptr;
  if (hipMalloc(d_ptr, bytes ? bytes : 1) != hipSuccess) {
    set_err(h, "pm_device_malloc: %zu bytes", bytes);
    return PM_ERR_NOMEM;
  }
  return PM_OK;
}

int pm_device_free(pm_handle* h, void* d_ptr) {
  if (!h) return PM_ERR_INVALID_ARG;
  if (!d_ptr) return PM_OK;
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  PM_HIP(h, hipStreamSynchronize(pm_internal::stream(h)));
  PM_HIP(h, hipFree(d_ptr));
  return PM_OK;
}

int pm_upload(pm_handle* h, void* d_dst, const void* src, size_t bytes) {
  if (!h || !d_dst || !src) return PM_ERR_INVALID_ARG;
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  PM_HIP(h, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, pm_internal::stream(h)));
  PM_HIP(h, hipStreamSynchronize(pm_internal::stream(h)));  // pageable source: the caller may reuse it right away
  return PM_OK;
}

int pm_download(pm_handle* h, void* dst, const void* d_src, size_t bytes) {
  if (!h || !dst || !d_src) return PM_ERR_INVALID_ARG;
  PM_HIP(h, hipSetDevice(pm_internal::device(h)));
  PM_HIP(h, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, pm_internal::stream(h)));
  PM_HIP(h, hipStreamSynchronize(pm_internal::stream(h)));
  return PM_OK;
}
