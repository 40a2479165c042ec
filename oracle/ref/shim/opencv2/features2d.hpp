// Stand-in: nothing of features2d is needed by the PatchMatch path.
#pragma once
#include "opencv2/core.hpp"
