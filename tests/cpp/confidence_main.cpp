// Drives DisparityConfidence of the C++ mirror (ocean-perception_amd/host/imaging.hpp) like a host caller.  Reads raw inputs
// written by tests/test_cpp_confidence.py and writes raw outputs for it to compare with the definition
// (tests/confidence_ref.py).
//   confidence_main <dir> <rows> <cols> <patch>   in: left.u8, right.u8, disp_l.f32, disp_r.f32;  out: out.f32, cost.f32,
//                                                 margin.f32, bg_margin.f32, lr.f32, flags.u8, counts.i32 (max_cost 10,
//                                                 min_margin 2, min_bg_margin 5, max_lr_diff 1), and out_only.f32 /
//                                                 out_only_counts.i32 of a call without the right map that asks for the
//                                                 map alone, with drop_unmeasured
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "imaging.hpp"
#include "raw_io.hpp"

using namespace bm::imaging;

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const std::string dir = argv[1];
  const int rows = atoi(argv[2]), cols = atoi(argv[3]), patch = atoi(argv[4]);
  if (rows < 1 || cols < 1) return 2;
  try {
    bm::core::Image<uint8_t> left(rows, cols), right(rows, cols);
    bm::core::Image<float> disp_l(rows, cols), disp_r(rows, cols);
    if (!read_raw(dir + "/left.u8", left) || !read_raw(dir + "/right.u8", right) || !read_raw(dir + "/disp_l.f32", disp_l) ||
        !read_raw(dir + "/disp_r.f32", disp_r)) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    ConfidenceOptions options;
    options.patch_w = options.patch_h = patch;
    options.max_cost = 10.f, options.min_margin = 2.f, options.min_bg_margin = 5.f, options.max_lr_diff = 1.f;
    bm::core::Image<float> out, out_only;
    ConfidenceMeasures measures;
    bm::core::Image<uint8_t> flags;
    bm::pm::PatchmatchGpu unplanned{bm::pm::PatchmatchGpu::Params()};
    try {
      DisparityConfidence(unplanned, left, right, options, disp_l, &disp_r, &out);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    bm::pm::PatchmatchGpu::Params params;
    params.max_rows = rows, params.max_cols = cols;
    bm::pm::PatchmatchGpu matcher(params);
    const std::array<int, 3> counts = DisparityConfidence(matcher, left, right, options, disp_l, &disp_r, &out, &measures, &flags);
    write_raw(dir + "/out.f32", out);
    write_raw(dir + "/cost.f32", measures.cost);
    write_raw(dir + "/margin.f32", measures.margin);
    write_raw(dir + "/bg_margin.f32", measures.bg_margin);
    write_raw(dir + "/lr.f32", measures.lr);
    write_raw(dir + "/flags.u8", flags);
    write_raw(dir + "/counts.i32", counts.data(), 3);
    options.drop_unmeasured = true;
    const std::array<int, 3> again = DisparityConfidence(matcher, left, right, options, disp_l, nullptr, &out_only);
    write_raw(dir + "/out_only.f32", out_only);
    write_raw(dir + "/out_only_counts.i32", again.data(), 3);
    options.patch_w = 4;
    try {
      DisparityConfidence(matcher, left, right, options, disp_l, &disp_r, &out);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    options.patch_w = patch;
    bm::core::Image<uint8_t> smaller(rows, cols - 1 > 0 ? cols - 1 : 1);
    try {
      DisparityConfidence(matcher, left, smaller, options, disp_l, &disp_r, &out);
      return 6;
    } catch (const std::invalid_argument& e) {
      std::printf("refused: %s\n", e.what());
    }
    std::printf("ok valid=%d measured=%d kept=%d\n", counts[0], counts[1], counts[2]);
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
