// Drives the C++ mirror of the range-guided illuminant (ocean-perception_amd/host/imaging.hpp) the way
// imaging::EnhanceUnderwater calls it (src/vehicle/imaging/enhance.cpp:59-63): host images in, host images out.
// Reads raw inputs written by tests/test_guided.py and writes raw outputs for it to compare with the fixture.
// usage: guided_main <dir> <rows> <cols> <r> <eps> <s>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "imaging.hpp"
#include "raw_io.hpp"

using namespace bm::imaging;

int main(int argc, char** argv) {
  if (argc < 7) return 2;
  const std::string dir = argv[1];
  const int rows = atoi(argv[2]), cols = atoi(argv[3]), r = atoi(argv[4]), s = atoi(argv[6]);
  const double eps = atof(argv[5]);
  try {
    Image3f D(rows, cols);
    Image1f range(rows, cols);
    if (!read_raw(dir + "/bgr.f32", D) || !read_raw(dir + "/range.f32", range)) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    write_raw(dir + "/il.f32", EstimateIlluminantRangeGuided(D, range, r, eps, s));
    write_raw(dir + "/lsac.f32", fastGuidedFilter(range, D, r, eps, s));
    Image1f first(rows, cols);
    for (int y = 0; y < rows; ++y)
      for (int x = 0; x < cols; ++x) first.at(y, x) = D.at(y, x).v[0];
    write_raw(dir + "/gray.f32", fastGuidedFilter(range, first, r, eps, s));
    std::printf("ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
