// The computing half of the OpenCV 3.4 stand-in (shim/opencv2/*.hpp).  TEST INFRASTRUCTURE ONLY; this project's own
// text, written independently of oracle/pm_oracle.c.  Always compiled with -ffp-contract=off, also for the contracted
// build of the reference: OpenCV is a separate library whose float code (SSE) has one rounding per operation.
#include "opencv2/core.hpp"
#include "opencv2/imgproc.hpp"

namespace cv {

void Mat::convertTo(Mat& dst, int rtype, double alpha, double beta) const {
  if (alpha != 1 || beta != 0) standin_abort("convertTo with a scale or an offset");
  const int ddepth = CV_MAT_DEPTH(rtype);
  if (channels() != 1) standin_abort("convertTo on several channels");
  if (ddepth == depth()) {
    Mat c = clone();
    dst = c;
    return;
  }
  Mat out(rows, cols, CV_MAKETYPE(ddepth, 1));
  for (int r = 0; r < rows; ++r) {
    if (depth() == CV_32F && ddepth == CV_8U) {
      const float* s = ptr<float>(r);
      uchar* d = out.ptr<uchar>(r);
      for (int c = 0; c < cols; ++c) d[c] = saturate_cast<uchar>(s[c]);
    } else if (depth() == CV_8U && ddepth == CV_32F) {
      const uchar* s = ptr<uchar>(r);
      float* d = out.ptr<float>(r);
      for (int c = 0; c < cols; ++c) d[c] = (float)s[c];
    } else {
      standin_abort("convertTo between these depths");
    }
  }
  dst = out;
}

// ---- element-wise arithmetic (core/arithm) ------------------------------------------------------------------------
namespace standin {
inline void same_shape(const Mat& a, const Mat& b, const char* what) {
  if (a.rows != b.rows || a.cols != b.cols || a.type() != b.type() || a.channels() != 1) standin_abort(what);
}
}  // namespace standin

// cv::add on 32f, with or without a mask; dst may be one of the sources (it keeps its storage then)
void add(const Mat& a, const Mat& b, Mat& dst, const Mat& mask) {
  standin::same_shape(a, b, "add on unequal operands");
  if (a.depth() != CV_32F) standin_abort("add on a depth other than 32f");
  Mat s1(a), s2(b);  // keep the operands alive if dst is re-created
  dst.create(a.rows, a.cols, a.type());
  const bool masked = !mask.empty();
  if (masked && (mask.rows != a.rows || mask.cols != a.cols || mask.type() != CV_8UC1)) standin_abort("add: mask shape");
  for (int r = 0; r < a.rows; ++r) {
    const float* p = s1.ptr<float>(r);
    const float* q = s2.ptr<float>(r);
    float* d = dst.ptr<float>(r);
    const uchar* m = masked ? mask.ptr<uchar>(r) : nullptr;
    for (int c = 0; c < a.cols; ++c)
      if (!m || m[c]) d[c] = p[c] + q[c];
  }
}

Mat operator+(const Mat& a, const Mat& b) {
  Mat out;
  add(a, b, out);
  return out;
}

// cv::max(Mat, scalar): the scalar is brought to the matrix depth first
Mat max(const Mat& a, double s) {
  if (a.type() != CV_32FC1) standin_abort("max on a type other than 32FC1");
  Mat out(a.rows, a.cols, a.type());
  const float fs = (float)s;
  for (int r = 0; r < a.rows; ++r) {
    const float* p = a.ptr<float>(r);
    float* d = out.ptr<float>(r);
    for (int c = 0; c < a.cols; ++c) d[c] = p[c] > fs ? p[c] : fs;
  }
  return out;
}

// Mat > scalar: cv::compare(CMP_GT), 255 where true
Mat operator>(const Mat& a, double s) {
  if (a.channels() != 1) standin_abort("compare on several channels");
  Mat out(a.rows, a.cols, CV_8UC1);
  for (int r = 0; r < a.rows; ++r) {
    uchar* d = out.ptr<uchar>(r);
    for (int c = 0; c < a.cols; ++c) {
      double v;
      switch (a.depth()) {
        case CV_8U: v = a.ptr<uchar>(r)[c]; break;
        case CV_32F: v = a.ptr<float>(r)[c]; break;
        case CV_64F: v = a.ptr<double>(r)[c]; break;
        default: standin_abort("compare on this depth");
      }
      d[c] = v > s ? 255 : 0;
    }
  }
  return out;
}

Mat operator*(const Mat&, const Mat&) { standin_abort("Mat * Mat"); }

void absdiff(const Mat& a, const Mat& b, Mat& dst) {
  standin::same_shape(a, b, "absdiff on unequal operands");
  Mat out(a.rows, a.cols, a.type());
  for (int r = 0; r < a.rows; ++r) {
    if (a.depth() == CV_8U) {
      const uchar *p = a.ptr<uchar>(r), *q = b.ptr<uchar>(r);
      uchar* d = out.ptr<uchar>(r);
      for (int c = 0; c < a.cols; ++c) d[c] = (uchar)(p[c] > q[c] ? p[c] - q[c] : q[c] - p[c]);
    } else if (a.depth() == CV_32F) {
      const float *p = a.ptr<float>(r), *q = b.ptr<float>(r);
      float* d = out.ptr<float>(r);
      for (int c = 0; c < a.cols; ++c) d[c] = std::fabs(p[c] - q[c]);
    } else {
      standin_abort("absdiff on this depth");
    }
  }
  dst = out;
}

// cv::mean: sum * (1. / N), a Scalar of doubles.  8u sums in int (exact); 32f sums four neighbours in float and
// adds that to a double accumulator, row after row (the generic sum_<float, double> loop).  On the PatchMatch path
// the 32f case only ever sees whole numbers up to 255, where every order of summation gives the same sum.
Scalar mean(const Mat& m) {
  if (m.channels() != 1) standin_abort("mean on several channels");
  const size_t n = (size_t)m.rows * m.cols;
  double total = 0;
  if (m.depth() == CV_8U) {
    long long isum = 0;
    for (int r = 0; r < m.rows; ++r) {
      const uchar* p = m.ptr<uchar>(r);
      for (int c = 0; c < m.cols; ++c) isum += p[c];
    }
    total = (double)isum;
  } else if (m.depth() == CV_32F) {
    // a continuous matrix is summed as one long row
    const int runs = m.isContinuous() ? 1 : m.rows;
    const int len = m.isContinuous() ? (int)n : m.cols;
    for (int r = 0; r < runs; ++r) {
      const float* p = m.ptr<float>(r);
      int c = 0;
      for (; c <= len - 4; c += 4) total += p[c] + p[c + 1] + p[c + 2] + p[c + 3];
      for (; c < len; ++c) total += p[c];
    }
  } else {
    standin_abort("mean on this depth");
  }
  return Scalar(total * (n > 0 ? 1. / (double)n : 0));
}

void meanStdDev(const Mat&, Scalar&, Scalar&) { standin_abort("meanStdDev"); }
void minMaxLoc(const Mat&, double*, double*) { standin_abort("minMaxLoc"); }

// cv::pow: a whole power of 2 is a multiplication
void pow(const Mat& src, double power, Mat& dst) {
  if (power != 2 || src.type() != CV_32FC1) standin_abort("pow other than 32f squared");
  Mat s(src);
  dst.create(src.rows, src.cols, src.type());
  for (int r = 0; r < s.rows; ++r) {
    const float* p = s.ptr<float>(r);
    float* d = dst.ptr<float>(r);
    for (int c = 0; c < s.cols; ++c) d[c] = p[c] * p[c];
  }
}

// cv::sqrt on 32f: the correctly rounded square root (sqrtps)
void sqrt(const Mat& src, Mat& dst) {
  if (src.type() != CV_32FC1) standin_abort("sqrt on a type other than 32FC1");
  Mat s(src);
  dst.create(src.rows, src.cols, src.type());
  for (int r = 0; r < s.rows; ++r) {
    const float* p = s.ptr<float>(r);
    float* d = dst.ptr<float>(r);
    for (int c = 0; c < s.cols; ++c) d[c] = std::sqrt(p[c]);
  }
}

namespace standin {

// One output sample of getRectSubPix.  The window's top-left sample lies at centre - (size - 1) / 2; (ix, iy) is
// its floor and (a, b) the fraction.  Rows are clamped to the image.  A column pair that lies inside the image is
// blended with the four products w00..w11; a sample whose left tap would fall before column 0, or whose right tap
// beyond the last column, takes that border column alone, blended vertically with (v0, v1) -- OpenCV's border branch.
template <typename T, typename W, class Finish>
inline void rect_subpix(const Mat& src, Size win, Mat& dst, W w00, W w01, W w10, W w11, W v0, W v1, int ix, int iy,
                        Finish finish) {
  const int H = src.rows, Wd = src.cols;
  for (int i = 0; i < win.height; ++i) {
    int y0 = iy + i, y1 = iy + i + 1;
    y0 = y0 < 0 ? 0 : y0 > H - 1 ? H - 1 : y0;
    y1 = y1 < 0 ? 0 : y1 > H - 1 ? H - 1 : y1;
    const T* r0 = src.ptr<T>(y0);
    const T* r1 = src.ptr<T>(y1);
    T* out = dst.ptr<T>(i);
    for (int j = 0; j < win.width; ++j) {
      const int x = ix + j;
      W s;
      if (x < 0)
        s = r0[0] * v0 + r1[0] * v1;
      else if (x >= Wd - 1)
        s = r0[Wd - 1] * v0 + r1[Wd - 1] * v1;
      else
        s = r0[x] * w00 + r0[x + 1] * w01 + r1[x] * w10 + r1[x + 1] * w11;
      out[j] = finish(s);
    }
  }
}

inline int reflect101(int p, int len) {
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

}  // namespace standin

// cv::getRectSubPix, one channel: 8u -> 8u (16-bit fixed-point weights, rounded) and 32f -> 32f
void getRectSubPix(const Mat& image, Size patchSize, Point2f center, Mat& patch, int patchType) {
  const int depth = image.depth();
  const int ddepth = patchType < 0 ? depth : CV_MAT_DEPTH(patchType);
  if (image.channels() != 1 || depth != ddepth || (depth != CV_8U && depth != CV_32F))
    standin_abort("getRectSubPix other than 8u -> 8u or 32f -> 32f on one channel");
  Mat src(image);
  patch.create(patchSize, image.type());
  center.x -= (patchSize.width - 1) * 0.5f;
  center.y -= (patchSize.height - 1) * 0.5f;
  const int ix = cvFloor(center.x), iy = cvFloor(center.y);
  const float a = center.x - ix, b = center.y - iy;
  const float f00 = (1.f - a) * (1.f - b), f01 = a * (1.f - b), f10 = (1.f - a) * b, f11 = a * b;
  if (depth == CV_8U) {
    const float one = (float)(1 << 16);
    standin::rect_subpix<uchar, int>(src, patchSize, patch, cvRound(f00 * one), cvRound(f01 * one),
                                     cvRound(f10 * one), cvRound(f11 * one), cvRound((1.f - b) * one),
                                     cvRound(b * one), ix, iy,
                                     [](int s) { return (uchar)((s + (1 << 15)) >> 16); });
  } else {
    standin::rect_subpix<float, float>(src, patchSize, patch, f00, f01, f10, f11, 1.f - b, b, ix, iy,
                                       [](float s) { return s; });
  }
}

// cv::Sobel, 8u -> 32f, aperture 3, first derivative in one direction, no scale: [-1 0 1] along the derivative axis and
// [1 2 1] across it, BORDER_REFLECT_101.  The taps are whole numbers, so the float result is exact.
void Sobel(const Mat& src, Mat& dst, int ddepth, int dx, int dy, int ksize, double scale, double delta,
           int borderType) {
  if (src.type() != CV_8UC1 || ddepth != CV_32F || ksize != 3 || scale != 1 || delta != 0 ||
      borderType != BORDER_REFLECT_101 || !((dx == 1 && dy == 0) || (dx == 0 && dy == 1)))
    standin_abort("Sobel other than 8u -> 32f, 3x3, first derivative, REFLECT_101");
  Mat s(src);
  Mat out(s.rows, s.cols, CV_32FC1);
  static const int deriv[3] = {-1, 0, 1}, smooth[3] = {1, 2, 1};
  const int* kx = dx ? deriv : smooth;
  const int* ky = dy ? deriv : smooth;
  for (int r = 0; r < s.rows; ++r) {
    float* d = out.ptr<float>(r);
    for (int c = 0; c < s.cols; ++c) {
      int acc = 0;
      for (int u = -1; u <= 1; ++u) {
        const uchar* row = s.ptr<uchar>(standin::reflect101(r + u, s.rows));
        for (int v = -1; v <= 1; ++v) acc += ky[u + 1] * kx[v + 1] * row[standin::reflect101(c + v, s.cols)];
      }
      d[c] = (float)acc;
    }
  }
  dst = out;
}

// RNG::fill(UNIFORM) on 32f; the formula is stated at its declaration (shim/opencv2/core.hpp)
void RNG::fill(Mat& m, int distType, double a, double b, bool saturateRange) {
  if (distType != UNIFORM || m.type() != CV_32FC1) standin_abort("RNG::fill other than UNIFORM on 32FC1");
  const double limit = saturateRange ? (double)FLT_MAX : DBL_MAX;
  const double span = b - a;
  const float scale = (float)((limit < span ? limit : span) * 2.3283064365386962890625e-10);
  const float mid = (float)((b + a) * 0.5);
  for (int r = 0; r < m.rows; ++r) {
    float* d = m.ptr<float>(r);
    for (int c = 0; c < m.cols; ++c) {
      const float prod = (float)(int)next() * scale;
      d[c] = prod + mid;
    }
  }
}

}  // namespace cv
