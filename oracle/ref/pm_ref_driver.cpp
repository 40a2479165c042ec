// C ABI over the reference's own CPU PatchMatch, compiled from the reference tree (oracle/ref/README.md).
//
// TEST INFRASTRUCTURE ONLY.  This translation unit #includes the reference's test file by path (PM_REF_TEST_FILE, set by
// the Makefile): its cost functor and its gradient routine are `static` and reachable in no other way.  The gtest
// stand-in turns the test body into a function that nothing calls.  stereo_matching/patchmatch.cpp is compiled as an
// object of its own (both files define a static VisualizeDisp).  Every pmr_* entry point mirrors a pmo_* one of
// oracle/pm_oracle.h; the last group exports the OpenCV stand-in's primitives so that they can be tested by themselves.
#include PM_REF_TEST_FILE

#include <cstdint>
#include <cstring>

namespace {

template <typename T> cv::Mat_<T> wrap(const T* src, int rows, int cols) {
  cv::Mat_<T> m(rows, cols);
  for (int r = 0; r < rows; ++r) std::memcpy(m.template ptr<T>(r), src + (size_t)r * cols, sizeof(T) * cols);
  return m;
}

template <typename T> void unwrap(const cv::Mat& m, T* dst) {
  if (m.type() != (int)cv::DataType<T>::type) std::abort();
  for (int r = 0; r < m.rows; ++r) std::memcpy(dst + (size_t)r * m.cols, m.ptr<T>(r), sizeof(T) * m.cols);
}

// The functor as Propagate receives it: a std::function with f32 gradient arguments around a function that takes
// them as 8-bit images -- the call goes through the converting Mat_ constructor.
const CostFunctor2& functor() {
  static const CostFunctor2 f = L1GradientCostFunction;
  return f;
}

Patchmatch& matcher() {
  static Patchmatch::Params params;
  static Patchmatch pm(params);
  return pm;
}

}  // namespace

extern "C" {

void pmr_add_noise(float* disp, int rows, int cols, float amount, const uint8_t* mask) {
  Image1f d = wrap(disp, rows, cols);
  Image1b m;
  if (mask) m = wrap(mask, rows, cols);
  matcher().AddNoise(d, amount, m);
  unwrap(d, disp);
}

void pmr_compute_gradient(const uint8_t* im, int rows, int cols, float* g) {
  Image1f gmag;
  ComputeGradient(wrap(im, rows, cols), gmag);
  unwrap(gmag, g);
}

float pmr_functor(const uint8_t* pl, const uint8_t* pr, const float* gl, const float* gr, int ph, int pw) {
  const Image1b a = wrap(pl, ph, pw), b = wrap(pr, ph, pw);
  const Image1f ga = wrap(gl, ph, pw), gb = wrap(gr, ph, pw);
  return functor()(a, b, ga, gb);
}

void pmr_propagate(const uint8_t* il, const uint8_t* ir, const float* gl, const float* gr, int rows, int cols,
                   float* disp, int ph, int pw) {
  Image1f d = wrap(disp, rows, cols);
  matcher().Propagate(wrap(il, rows, cols), wrap(ir, rows, cols), wrap(gl, rows, cols), wrap(gr, rows, cols), d,
                      functor(), ph, pw);
  unwrap(d, disp);
}

void pmr_remove_background(const uint8_t* il, const uint8_t* ir, const float* gl, const float* gr, int rows, int cols,
                           float* disp, int ph, int pw, float factor) {
  Image1f d = wrap(disp, rows, cols);
  matcher().RemoveBackground(wrap(il, rows, cols), wrap(ir, rows, cols), wrap(gl, rows, cols), wrap(gr, rows, cols),
                             d, functor(), ph, pw, factor);
  unwrap(d, disp);
}

// As above with the header's default factor (the argument is left out of the call).
void pmr_remove_background_default(const uint8_t* il, const uint8_t* ir, const float* gl, const float* gr, int rows,
                                   int cols, float* disp, int ph, int pw) {
  Image1f d = wrap(disp, rows, cols);
  matcher().RemoveBackground(wrap(il, rows, cols), wrap(ir, rows, cols), wrap(gl, rows, cols), wrap(gr, rows, cols),
                             d, functor(), ph, pw);
  unwrap(d, disp);
}

// The schedule the reference's test runs after seeding: four rounds of masked noise and a four-pass propagation, with
// a shrinking amplitude and window, then the background test.  disp holds the seed map on entry, the result on return.
void pmr_recipe(const uint8_t* il, const uint8_t* ir, int rows, int cols, float* disp) {
  static const struct { float amount; int window; } rounds[4] = {{32.0f, 5}, {8.0f, 5}, {2.0f, 3}, {0.5f, 3}};
  const Image1b l = wrap(il, rows, cols), r = wrap(ir, rows, cols);
  Image1f gl, gr;
  ComputeGradient(l, gl);
  ComputeGradient(r, gr);
  Image1f d = wrap(disp, rows, cols);
  Patchmatch& pm = matcher();
  for (const auto& round : rounds) {
    pm.AddNoise(d, round.amount, d > 0);
    pm.Propagate(l, r, gl, gr, d, functor(), round.window, round.window);
  }
  pm.RemoveBackground(l, r, gl, gr, d, functor(), 3, 3, 1.5);
  unwrap(d, disp);
}

// ---- the stand-in's primitives ----------------------------------------------------------------------------------------
void pmr_rect_subpix_u8(const uint8_t* src, int rows, int cols, int pw, int ph, float cx, float cy, uint8_t* dst) {
  cv::Mat1b patch;
  cv::getRectSubPix(wrap(src, rows, cols), cv::Size(pw, ph), cv::Point2f(cx, cy), patch);
  unwrap(patch, dst);
}

void pmr_rect_subpix_f32(const float* src, int rows, int cols, int pw, int ph, float cx, float cy, float* dst) {
  cv::Mat1f patch;
  cv::getRectSubPix(wrap(src, rows, cols), cv::Size(pw, ph), cv::Point2f(cx, cy), patch);
  unwrap(patch, dst);
}

void pmr_rng_raw(uint32_t* dst, size_t n, uint64_t seed) {
  cv::RNG rng(seed);
  for (size_t i = 0; i < n; ++i) dst[i] = rng.next();
}

void pmr_rng_fill(float* dst, int rows, int cols, double lo, double hi, int saturate_range, uint64_t seed) {
  cv::Mat1f m(rows, cols);
  cv::RNG rng(seed);
  rng.fill(m, cv::RNG::UNIFORM, lo, hi, saturate_range != 0);
  unwrap(m, dst);
}

void pmr_sobel(const uint8_t* im, int rows, int cols, int dx, int dy, float* dst) {
  cv::Mat out;
  cv::Sobel(wrap(im, rows, cols), out, CV_32F, dx, dy, 3);
  unwrap(out, dst);
}

double pmr_mean_u8(const uint8_t* src, int rows, int cols) { return cv::mean(wrap(src, rows, cols))[0]; }
double pmr_mean_f32(const float* src, int rows, int cols) { return cv::mean(wrap(src, rows, cols))[0]; }

void pmr_convert_f32_u8(const float* src, int rows, int cols, uint8_t* dst) {
  const cv::Mat1b converted(cv::Mat(wrap(src, rows, cols)));
  unwrap(converted, dst);
}

// 1 if this library was built with the reference's own options (contraction allowed), 0 for -ffp-contract=off
int pmr_contracted(void) {
#ifdef PM_REF_CONTRACTED
  return 1;
#else
  return 0;
#endif
}

}  // extern "C"
