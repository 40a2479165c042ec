// Stand-in for opencv2/imgproc.hpp: getRectSubPix and Sobel compute (OpenCV 3.4 semantics); the rest is declared only.
#pragma once

#include "opencv2/core.hpp"

namespace cv {

enum { BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_REFLECT_101 = 4, BORDER_DEFAULT = 4 };
enum { INTER_NEAREST = 0, INTER_LINEAR = 1, INTER_CUBIC = 2, INTER_AREA = 3 };
enum { MORPH_RECT = 0, MORPH_CROSS = 1, MORPH_ELLIPSE = 2 };
enum { MORPH_ERODE = 0, MORPH_DILATE = 1, MORPH_OPEN = 2, MORPH_CLOSE = 3, MORPH_GRADIENT = 4 };
enum { COLORMAP_JET = 2, COLORMAP_PARULA = 12 };

// defined in oracle/ref/cv_standin.cpp
void getRectSubPix(const Mat& image, Size patchSize, Point2f center, Mat& patch, int patchType = -1);
void Sobel(const Mat& src, Mat& dst, int ddepth, int dx, int dy, int ksize = 3, double scale = 1, double delta = 0,
           int borderType = BORDER_DEFAULT);

inline Mat getStructuringElement(int, Size, Point = Point(-1, -1)) { standin_abort("getStructuringElement"); }
inline void resize(const Mat&, Mat&, Size, double = 0, double = 0, int = INTER_LINEAR) { standin_abort("resize"); }
inline void dilate(const Mat&, Mat&, const Mat&, Point = Point(-1, -1), int = 1) { standin_abort("dilate"); }
inline void morphologyEx(const Mat&, Mat&, int, const Mat&, Point = Point(-1, -1), int = 1) {
  standin_abort("morphologyEx");
}
inline void applyColorMap(const Mat&, Mat&, int) { standin_abort("applyColorMap"); }

}  // namespace cv
