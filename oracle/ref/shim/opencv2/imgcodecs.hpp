// Stand-in for opencv2/imgcodecs.hpp: declared for compilation only.
#pragma once
#include "opencv2/core.hpp"

namespace cv {
enum { IMREAD_GRAYSCALE = 0, IMREAD_COLOR = 1 };
inline Mat imread(const std::string&, int = IMREAD_COLOR) { standin_abort("imread"); }
}  // namespace cv
