// Drives FilterConsistency of the C++ mirror (ocean-perception_amd/host/imaging.hpp) like a host caller.  Reads raw inputs
// written by tests/test_cpp_consistency.py and writes raw outputs for it to compare with the definition
// (tests/consistency_ref.py).
//   consistency_main <dir> <rows> <cols> <n>   in: disp.f32 (the current left map), sources.f32 ([n][rows][cols]),
//                                              motions.f64 (n x (R[9], t[3]));  out: out.f32, classes.u16, residual.f32,
//                                              counts.i32 (max_diff 0.75, radius 1, min_consistent 2, max_conflicts 0), and
//                                              out_only.f32 / out_only_counts.i32 of a call that asks for the map alone
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "imaging.hpp"
#include "raw_io.hpp"

using namespace bm::imaging;

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const std::string dir = argv[1];
  const int rows = atoi(argv[2]), cols = atoi(argv[3]), n = atoi(argv[4]);
  if (rows < 1 || cols < 1 || n < 1) return 2;
  try {
    bm::core::Image<float> disp(rows, cols);
    std::vector<bm::core::Image<float>> sources;
    std::vector<float> all((size_t)n * rows * cols);
    std::vector<double> mv((size_t)n * 12);
    if (!read_raw(dir + "/disp.f32", disp) || !read_raw(dir + "/sources.f32", all.data(), all.size()) ||
        !read_raw(dir + "/motions.f64", mv.data(), mv.size())) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    std::vector<Motion> motions((size_t)n);
    for (int k = 0; k < n; ++k) {
      sources.emplace_back(rows, cols);
      std::copy(all.begin() + (size_t)k * rows * cols, all.begin() + (size_t)(k + 1) * rows * cols, sources.back().data());
      for (size_t i = 0; i < 9; ++i) motions[(size_t)k].R[i] = mv[(size_t)k * 12 + i];
      for (size_t i = 0; i < 3; ++i) motions[(size_t)k].t[i] = mv[(size_t)k * 12 + 9 + i];
    }
    StereoModel model;
    model.fx = 412.7, model.fy = 398.3, model.cx = cols / 2 - 0.3, model.cy = rows / 2 + 0.4, model.baseline = 0.12;
    ConsistencyOptions options;
    options.max_diff = 0.75f;
    options.min_consistent = 2;
    bm::core::Image<float> out, residual, out_only;
    bm::core::Image<uint16_t> classes;
    bm::pm::PatchmatchGpu unplanned{bm::pm::PatchmatchGpu::Params()};
    try {
      FilterConsistency(unplanned, model, sources, motions, options, disp, &out);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    bm::pm::PatchmatchGpu::Params params;
    params.max_rows = rows, params.max_cols = cols;
    bm::pm::PatchmatchGpu matcher(params);
    const std::array<int, 2> counts = FilterConsistency(matcher, model, sources, motions, options, disp, &out, &classes, &residual);
    write_raw(dir + "/out.f32", out);
    write_raw(dir + "/classes.u16", classes);
    write_raw(dir + "/residual.f32", residual);
    write_raw(dir + "/counts.i32", counts.data(), 2);
    const std::array<int, 2> again = FilterConsistency(matcher, model, sources, motions, options, disp, &out_only);
    write_raw(dir + "/out_only.f32", out_only);
    write_raw(dir + "/out_only_counts.i32", again.data(), 2);
    options.radius = 3;
    try {
      FilterConsistency(matcher, model, sources, motions, options, disp, &out);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    options.radius = 1;
    motions.pop_back();
    try {
      FilterConsistency(matcher, model, sources, motions, options, disp, &out);
      return 6;
    } catch (const std::invalid_argument& e) {
      std::printf("refused: %s\n", e.what());
    }
    std::printf("ok valid=%d kept=%d\n", counts[0], counts[1]);
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
