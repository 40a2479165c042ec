// Stand-in for opencv2/highgui.hpp: declared for compilation only.
#pragma once
#include "opencv2/core.hpp"
#include "opencv2/imgcodecs.hpp"

namespace cv {
enum { WINDOW_NORMAL = 0, WINDOW_AUTOSIZE = 1 };
inline void namedWindow(const std::string&, int = WINDOW_AUTOSIZE) { standin_abort("namedWindow"); }
inline void imshow(const std::string&, const Mat&) { standin_abort("imshow"); }
inline int waitKey(int = 0) { standin_abort("waitKey"); }
}  // namespace cv
