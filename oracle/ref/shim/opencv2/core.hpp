// Stand-in for the part of OpenCV 3.4 that the reference's CPU PatchMatch touches (oracle/ref/README.md).
//
// TEST INFRASTRUCTURE ONLY.  This is this project's own text, written from OpenCV 3.4's published behaviour and
// independently of oracle/pm_oracle.c: the two restatements are compared bit for bit by tests/test_reference_build.py.
// What the PatchMatch path executes really computes (Mat storage and ROI, the converting Mat_ constructor, getRectSubPix,
// absdiff, mean, RNG::fill, add, max, compare, Sobel, pow, sqrt, Mat + Mat, Size / int).  Names that only code which
// never runs here mentions (imshow, imread, resize, dilate, ...) are declared and abort when called.
#pragma once

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <ostream>
#include <string>
#include <vector>

// depth / type codes and the old C constants are macros or global enumerators in OpenCV
enum { CV_8U = 0, CV_8S = 1, CV_16U = 2, CV_16S = 3, CV_32S = 4, CV_32F = 5, CV_64F = 6 };
#define CV_MAKETYPE(depth, cn) ((depth) + (((cn) - 1) << 3))
#define CV_MAT_DEPTH(type) ((type) & 7)
#define CV_MAT_CN(type) ((((type) >> 3) & 63) + 1)
enum {
  CV_8UC1 = CV_MAKETYPE(CV_8U, 1), CV_8UC3 = CV_MAKETYPE(CV_8U, 3), CV_32FC1 = CV_MAKETYPE(CV_32F, 1),
  CV_32FC3 = CV_MAKETYPE(CV_32F, 3), CV_64FC1 = CV_MAKETYPE(CV_64F, 1), CV_64FC3 = CV_MAKETYPE(CV_64F, 3)
};
enum { CV_LOAD_IMAGE_GRAYSCALE = 0 };

namespace cv {

typedef unsigned char uchar;

[[noreturn]] inline void standin_abort(const char* what) {
  std::fprintf(stderr, "OpenCV stand-in: %s is declared for compilation only and must not run\n", what);
  std::abort();
}

// ---- rounding ---------------------------------------------------------------------------------------------------
// cvRound is a conversion in the current (nearest-even) rounding mode: cvtss2si / cvtsd2si
inline int cvRound(float v) { return (int)std::lrintf(v); }
inline int cvRound(double v) { return (int)std::lrint(v); }
inline int cvFloor(float v) { int i = (int)v; return i - (v < (float)i); }
inline int cvFloor(double v) { int i = (int)v; return i - (v < (double)i); }

template <typename T> inline T saturate_cast(float v) { return (T)v; }
template <typename T> inline T saturate_cast(double v) { return (T)v; }
template <typename T> inline T saturate_cast(int v) { return (T)v; }
template <> inline uchar saturate_cast<uchar>(int v) { return (uchar)((unsigned)v <= 255u ? v : v > 0 ? 255 : 0); }
template <> inline uchar saturate_cast<uchar>(float v) { return saturate_cast<uchar>(cvRound(v)); }
template <> inline uchar saturate_cast<uchar>(double v) { return saturate_cast<uchar>(cvRound(v)); }

// ---- small value types ------------------------------------------------------------------------------------------
template <typename T> struct Point_ {
  T x, y;
  Point_() : x(0), y(0) {}
  Point_(T x_, T y_) : x(x_), y(y_) {}
};
typedef Point_<int> Point2i;
typedef Point_<float> Point2f;
typedef Point_<double> Point2d;
typedef Point2i Point;

template <typename T> struct Size_ {
  T width, height;
  Size_() : width(0), height(0) {}
  Size_(T w, T h) : width(w), height(h) {}
};
typedef Size_<int> Size;
template <typename T> inline bool operator==(const Size_<T>& a, const Size_<T>& b) {
  return a.width == b.width && a.height == b.height;
}
template <typename T> inline bool operator!=(const Size_<T>& a, const Size_<T>& b) { return !(a == b); }
template <typename T> inline Size_<T> operator/(const Size_<T>& a, T b) { return Size_<T>(a.width / b, a.height / b); }
template <typename T> inline Size_<T> operator*(const Size_<T>& a, T b) { return Size_<T>(a.width * b, a.height * b); }
template <typename T> inline std::ostream& operator<<(std::ostream& o, const Size_<T>& s) {
  return o << "[" << s.width << " x " << s.height << "]";
}

template <typename T> struct Rect_ {
  T x, y, width, height;
  Rect_() : x(0), y(0), width(0), height(0) {}
  Rect_(T x_, T y_, T w, T h) : x(x_), y(y_), width(w), height(h) {}
};
typedef Rect_<int> Rect;

template <typename T> struct Scalar_ {
  T val[4];
  Scalar_() : val{0, 0, 0, 0} {}
  Scalar_(T v0, T v1 = 0, T v2 = 0, T v3 = 0) : val{v0, v1, v2, v3} {}
  T& operator[](int i) { return val[i]; }
  const T& operator[](int i) const { return val[i]; }
};
typedef Scalar_<double> Scalar;

template <typename T, int N> struct Vec {
  T val[N];
};
typedef Vec<uchar, 3> Vec3b;
typedef Vec<float, 3> Vec3f;
typedef Vec<double, 3> Vec3d;

template <typename T> struct DataType;
template <> struct DataType<uchar> { enum { type = CV_8UC1 }; };
template <> struct DataType<float> { enum { type = CV_32FC1 }; };
template <> struct DataType<double> { enum { type = CV_64FC1 }; };
template <> struct DataType<Vec3b> { enum { type = CV_8UC3 }; };
template <> struct DataType<Vec3f> { enum { type = CV_32FC3 }; };
template <> struct DataType<Vec3d> { enum { type = CV_64FC3 }; };

class FileNode {};

// ---- Mat: a reference-counted 2-D array with a row stride, so that headers and ROIs share storage -----------------
class Mat {
 public:
  int rows, cols;
  size_t step;  // bytes per row
  uchar* data;

  Mat() : rows(0), cols(0), step(0), data(nullptr), type_(0), block_(nullptr) {}
  Mat(int r, int c, int type) : Mat() { create(r, c, type); }
  Mat(Size s, int type) : Mat() { create(s.height, s.width, type); }
  Mat(const Mat& m) : rows(m.rows), cols(m.cols), step(m.step), data(m.data), type_(m.type_), block_(m.block_) { retain(); }
  Mat(const Mat& m, const Rect& roi) : Mat(m) {
    if (roi.x < 0 || roi.y < 0 || roi.width < 0 || roi.height < 0 || roi.x + roi.width > m.cols ||
        roi.y + roi.height > m.rows)
      standin_abort("a ROI outside its matrix (OpenCV asserts)");
    data += (size_t)roi.y * step + (size_t)roi.x * elemSize();
    rows = roi.height;
    cols = roi.width;
  }
  ~Mat() { release(); }
  Mat& operator=(const Mat& m) {
    if (this != &m) {
      Mat keep(m);
      swap(keep);
    }
    return *this;
  }

  // as OpenCV: keeps the storage when size and type already fit
  void create(int r, int c, int type) {
    if (data && rows == r && cols == c && type_ == type) return;
    release();
    rows = r;
    cols = c;
    type_ = type;
    step = (size_t)c * elemSize();
    size_t bytes = step * (size_t)r;
    block_ = (Block*)std::malloc(sizeof(Block) + (bytes ? bytes : 1));
    if (!block_) std::abort();
    new (&block_->refs) std::atomic<int>(1);
    data = (uchar*)(block_ + 1);
  }
  void create(Size s, int type) { create(s.height, s.width, type); }

  int type() const { return type_; }
  int depth() const { return CV_MAT_DEPTH(type_); }
  int channels() const { return CV_MAT_CN(type_); }
  size_t elemSize() const {
    static const int bytes[7] = {1, 1, 2, 2, 4, 4, 8};
    return (size_t)bytes[depth()] * channels();
  }
  Size size() const { return Size(cols, rows); }
  bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
  bool isContinuous() const { return rows <= 1 || step == (size_t)cols * elemSize(); }

  template <typename T> T* ptr(int r = 0) { return (T*)(data + (size_t)r * step); }
  template <typename T> const T* ptr(int r = 0) const { return (const T*)(data + (size_t)r * step); }
  template <typename T> T& at(int r, int c) { return ptr<T>(r)[c]; }
  template <typename T> const T& at(int r, int c) const { return ptr<T>(r)[c]; }

  // Mat::convertTo without scaling: saturate_cast of every element (8u <-> 32f, the two the path uses)
  void convertTo(Mat& dst, int rtype, double alpha = 1, double beta = 0) const;
  Mat clone() const {
    Mat out(rows, cols, type_);
    for (int r = 0; r < rows; ++r) std::memcpy(out.ptr<uchar>(r), ptr<uchar>(r), (size_t)cols * elemSize());
    return out;
  }
  Mat& operator/=(double) { standin_abort("Mat /= scalar"); }

 protected:
  struct Block {
    std::atomic<int> refs;
    double align_;  // keeps the payload 8-byte aligned
  };
  int type_;
  Block* block_;
  void retain() {
    if (block_) block_->refs.fetch_add(1, std::memory_order_relaxed);
  }
  void release() {
    if (block_ && block_->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) std::free(block_);
    block_ = nullptr;
    data = nullptr;
    rows = cols = 0;
    step = 0;
  }
  void swap(Mat& o) {
    std::swap(rows, o.rows);
    std::swap(cols, o.cols);
    std::swap(step, o.step);
    std::swap(data, o.data);
    std::swap(type_, o.type_);
    std::swap(block_, o.block_);
  }
};

// Mat_<T>: the typed header.  Built from a Mat of another type it CONVERTS (Mat::convertTo, i.e. saturate_cast) --
// the implicit Mat_<float> -> Mat_<uchar> conversion that the reference's cost functor goes through.
template <typename T> class Mat_ : public Mat {
 public:
  Mat_() : Mat() { type_ = DataType<T>::type; }
  Mat_(int r, int c) : Mat(r, c, DataType<T>::type) {}
  explicit Mat_(Size s) : Mat(s, DataType<T>::type) {}
  Mat_(Size s, const T& value) : Mat(s, DataType<T>::type) { fill(value); }
  Mat_(int r, int c, const T& value) : Mat(r, c, DataType<T>::type) { fill(value); }
  Mat_(const Mat_& m) : Mat(m) {}
  Mat_(const Mat_& m, const Rect& roi) : Mat(m, roi) {}
  Mat_(const Mat& m) : Mat() {
    type_ = DataType<T>::type;
    *this = m;
  }
  Mat_& operator=(const Mat_& m) {
    Mat::operator=(m);
    return *this;
  }
  Mat_& operator=(const Mat& m) {
    if (m.type() == (int)DataType<T>::type || m.data == nullptr) {
      Mat::operator=(m);
      type_ = DataType<T>::type;
    } else {
      Mat converted;
      m.convertTo(converted, DataType<T>::type);
      Mat::operator=(converted);
    }
    return *this;
  }
  T& operator()(int r, int c) { return this->template at<T>(r, c); }
  const T& operator()(int r, int c) const { return this->template at<T>(r, c); }

 private:
  void fill(const T& v) {
    for (int r = 0; r < rows; ++r) {
      T* p = this->template ptr<T>(r);
      for (int c = 0; c < cols; ++c) p[c] = v;
    }
  }
};
typedef Mat_<uchar> Mat1b;
typedef Mat_<Vec3b> Mat3b;
typedef Mat_<float> Mat1f;
typedef Mat_<Vec3f> Mat3f;
typedef Mat_<double> Mat1d;
typedef Mat_<Vec3d> Mat3d;

// ---- element-wise arithmetic (core/arithm); defined in oracle/ref/cv_standin.cpp, which is always compiled with
// -ffp-contract=off: OpenCV is a library of its own, the flags of the code that calls it do not reach into it ---------
void add(const Mat& a, const Mat& b, Mat& dst, const Mat& mask = Mat());
Mat operator+(const Mat& a, const Mat& b);
Mat max(const Mat& a, double s);
Mat operator>(const Mat& a, double s);
Mat operator*(const Mat& a, const Mat& b);
void absdiff(const Mat& a, const Mat& b, Mat& dst);
Scalar mean(const Mat& m);
void meanStdDev(const Mat& m, Scalar& mean, Scalar& stddev);
void minMaxLoc(const Mat& m, double* lo, double* hi);
void pow(const Mat& src, double power, Mat& dst);
void sqrt(const Mat& src, Mat& dst);

// ---- cv::RNG: multiply-with-carry, and fill(UNIFORM) for 32f ----------------------------------------------------------
class RNG {
 public:
  enum { UNIFORM = 0, NORMAL = 1 };
  uint64_t state;
  RNG() : state(0xffffffff) {}
  RNG(uint64_t seed) : state(seed ? seed : 0xffffffff) {}
  unsigned next() {
    state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
    return (unsigned)state;
  }
  // every element is  (float)(int)next() * scale + mid  in binary32, a product and then a sum, with
  //   scale = (float)(min(limit, b - a) * 2^-32),  mid = (float)((b + a) / 2),
  // limit = FLT_MAX when saturateRange is set and DBL_MAX otherwise.
  void fill(Mat& m, int distType, double a, double b, bool saturateRange = false);
};

}  // namespace cv
