// Stand-in: cv::Mat lives in opencv2/core.hpp.
#pragma once
#include "opencv2/core.hpp"
