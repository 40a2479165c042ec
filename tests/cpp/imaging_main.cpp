// Drives the C++ mirror of the bm::imaging functions (ocean-perception_amd/host/imaging.hpp) the way the
// reference's tests call them (test/imaging/enhance_test.cpp:55-80, src/vehicle/imaging/enhance.cpp:22-85):
// host images in, host images out.  Reads raw inputs written by tests/test_cpp_imaging.py and writes raw outputs
// for it to check against the oracle.  usage: imaging_main <dir> <rows> <cols>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "imaging.hpp"
#include "raw_io.hpp"

using namespace bm::imaging;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::string dir = argv[1];
  const int rows = atoi(argv[2]), cols = atoi(argv[3]);
  try {
    Image3b raw(rows, cols);
    Image1f disp(rows, cols);
    if (!read_raw(dir + "/bgr.u8", raw) || !read_raw(dir + "/disp.f32", disp)) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    // enhance_test.cpp:61-73
    const Image3f I = CastImage3bTo3f(raw);
    const Image3f J = Normalize(NormalizeColorIlluminant(I));
    write_raw(dir + "/J.f32", J);
    write_raw(dir + "/gray8.u8", StereoReady(raw));
    // enhance.cpp:33-36, :56, :83 with fixed parameters (the LM fits are the caller's)
    const Image1f range = DispToDepth(disp, 400.0, 0.1);
    write_raw(dir + "/range.f32", range);
    const Image1f intensity = ComputeIntensity(I);
    Image1b is_dark;
    const float thr = FindDarkFast(intensity, range, 0.05f, is_dark);
    write_raw(dir + "/dark.u8", is_dark);
    const Vector3f B = {0.132f, 0.115f, 0.0559f}, beta_B = {0.358f, 0.695f, 1.11f};
    const Vector12f X = {0.30f, 0.25f, 0.40f, -0.20f, -0.15f, -0.30f, 0.10f, 0.12f, 0.08f, -0.05f, -0.04f, -0.06f};
    const Image3f D = RemoveBackscatter(I, range, B, beta_B);
    write_raw(dir + "/D.f32", D);
    write_raw(dir + "/out.f32", CorrectAttenuation(D, range, X));
    const int k = cols / 3 + (1 - (cols / 3) % 2);
    write_raw(dir + "/il.f32", EstimateIlluminantGaussian(I, k, k, k / 4.0f, k / 4.0f));
    std::printf("ok thr=%.9g\n", thr);
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
