// Drives DisparityNormals of the C++ mirror (ocean-perception_amd/host/imaging.hpp) like a host caller: a host map in, host
// images out.  Reads the raw input written by tests/test_cpp_normals_fit.py and writes raw outputs for it to compare with the
// definition (tests/normals_fit_ref.py).
//   normals_fit_main <dir> <rows> <cols>
// in:  disp.f32
// out: normals.f32, support.u8 (radius 5, max_diff 1, min_support 9: the defaults), normals_r2.f32 (radius 2, max_diff 30,
//      min_support 3, no support map)
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
    StereoModel model;
    model.fx = 412.7, model.fy = 398.3, model.cx = cols / 2 - 0.3, model.cy = rows / 2 + 0.4, model.baseline = 0.12;
    bm::core::Image<uint8_t> support;
    const bm::core::Image<bm::core::Vec3f> normals = DisparityNormals(disp, model, NormalsFit(), &support);
    if (normals.rows != rows || normals.cols != cols || support.rows != rows || support.cols != cols) return 4;
    write_raw(dir + "/normals.f32", normals.data(), px);
    write_raw(dir + "/support.u8", support.data(), px);
    NormalsFit fit;
    fit.radius = 2, fit.max_diff = 30.f, fit.min_support = 3;
    write_raw(dir + "/normals_r2.f32", DisparityNormals(disp, model, fit).data(), px);
    // what the C call refuses, the wrapper throws
    fit.radius = 8;
    try {
      DisparityNormals(disp, model, fit);
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
