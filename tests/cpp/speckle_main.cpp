// Drives FilterSpeckles of the C++ mirror (ocean-perception_amd/host/imaging.hpp) like a host caller: a host map in, host
// images out.  Reads the raw input written by tests/test_cpp_speckle.py and writes raw outputs for it to compare with the
// definition (tests/speckle_ref.py).
//   speckle_main <dir> <rows> <cols>
// in:  disp.f32
// out: out.f32, labels.i32, removed.i32 (max_diff 1, max_size 100: the defaults), out_small.f32 (max_diff 0.25, max_size 3,
//      no labels, no count)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

#include "imaging.hpp"
#include "raw_io.hpp"

using namespace bm::imaging;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::string dir = argv[1];
  const int rows = atoi(argv[2]), cols = atoi(argv[3]);
  const size_t px = (size_t)rows * cols;
  try {
    bm::core::Image<float> disp(rows, cols);
    std::ifstream f(dir + "/disp.f32", std::ios::binary);
    if (!f || !f.read(reinterpret_cast<char*>(disp.data()), sizeof(float) * px)) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    bm::core::Image<int32_t> labels;
    int removed = -1;
    const bm::core::Image<float> out = FilterSpeckles(disp, SpeckleFilter(), &labels, &removed);
    if (out.rows != rows || out.cols != cols || labels.rows != rows || labels.cols != cols) return 4;
    write_raw(dir + "/out.f32", out.data(), px);
    write_raw(dir + "/labels.i32", labels.data(), px);
    write_raw(dir + "/removed.i32", &removed, 1);
    SpeckleFilter filter;
    filter.max_diff = 0.25f, filter.max_size = 3;
    write_raw(dir + "/out_small.f32", FilterSpeckles(disp, filter).data(), px);
    // what the C call refuses, the wrapper throws
    filter.max_size = -1;
    try {
      FilterSpeckles(disp, filter);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    std::printf("ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
