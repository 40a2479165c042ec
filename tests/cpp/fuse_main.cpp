// Drives FuseDisparity of the C++ mirror (ocean-perception_amd/host/imaging.hpp) like a host caller.  Reads raw inputs
// written by tests/test_cpp_fuse.py and writes raw outputs for it to compare with the definition (tests/fuse_ref.py).
//   fuse_main <dir> <rows> <cols> <n>   in: disp.f32 (the current left map), sources.f32 ([n][rows][cols]), motions.f64
//                                       (n x (R[9], t[3])), weights.f32 ([2][rows][cols]: the current map's plane and source
//                                       0's; the other sources have none);  out: out.f32, count.u8, spread.f32, flags.u8,
//                                       counts.i32 (max_diff 0.75, radius 1, min_consistent 1, max_conflicts 8,
//                                       fill_min_sources 2, fill_max_diff 0.75), and out_only.f32 / out_only_counts.i32 of a
//                                       call without weights and without a fill that asks for the map alone
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
  if (rows < 1 || cols < 1 || n < 2) return 2;
  try {
    const size_t px = (size_t)rows * cols;
    bm::core::Image<float> disp(rows, cols), weight(rows, cols);
    std::vector<bm::core::Image<float>> sources, source_weights((size_t)n);
    std::vector<float> all((size_t)n * px), w(2 * px);
    std::vector<double> mv((size_t)n * 12);
    if (!read_raw(dir + "/disp.f32", disp) || !read_raw(dir + "/sources.f32", all.data(), all.size()) ||
        !read_raw(dir + "/motions.f64", mv.data(), mv.size()) || !read_raw(dir + "/weights.f32", w.data(), w.size())) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    std::copy(w.begin(), w.begin() + px, weight.data());
    source_weights[0].create(rows, cols);
    std::copy(w.begin() + px, w.end(), source_weights[0].data());
    std::vector<Motion> motions((size_t)n);
    for (int k = 0; k < n; ++k) {
      sources.emplace_back(rows, cols);
      std::copy(all.begin() + (size_t)k * px, all.begin() + (size_t)(k + 1) * px, sources.back().data());
      for (size_t i = 0; i < 9; ++i) motions[(size_t)k].R[i] = mv[(size_t)k * 12 + i];
      for (size_t i = 0; i < 3; ++i) motions[(size_t)k].t[i] = mv[(size_t)k * 12 + 9 + i];
    }
    StereoModel model;
    model.fx = 412.7, model.fy = 398.3, model.cx = cols / 2 - 0.3, model.cy = rows / 2 + 0.4, model.baseline = 0.12;
    FuseOptions options;
    options.max_diff = 0.75f;
    options.max_conflicts = 8;
    options.fill_min_sources = 2;
    options.fill_max_diff = 0.75f;
    bm::core::Image<float> out, spread, out_only;
    bm::core::Image<uint8_t> count, flags;
    bm::pm::PatchmatchGpu unplanned{bm::pm::PatchmatchGpu::Params()};
    try {
      FuseDisparity(unplanned, model, sources, motions, options, disp, &weight, source_weights, &out);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    bm::pm::PatchmatchGpu::Params params;
    params.max_rows = rows, params.max_cols = cols;
    bm::pm::PatchmatchGpu matcher(params);
    const std::array<int, 4> counts =
        FuseDisparity(matcher, model, sources, motions, options, disp, &weight, source_weights, &out, &count, &spread, &flags);
    write_raw(dir + "/out.f32", out);
    write_raw(dir + "/count.u8", count);
    write_raw(dir + "/spread.f32", spread);
    write_raw(dir + "/flags.u8", flags);
    write_raw(dir + "/counts.i32", counts.data(), 4);
    options.fill_min_sources = 0;
    const std::array<int, 4> again = FuseDisparity(matcher, model, sources, motions, options, disp, nullptr, {}, &out_only);
    write_raw(dir + "/out_only.f32", out_only);
    write_raw(dir + "/out_only_counts.i32", again.data(), 4);
    options.fill_min_sources = n + 1;
    try {
      FuseDisparity(matcher, model, sources, motions, options, disp, nullptr, {}, &out);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    options.fill_min_sources = 0;
    motions.pop_back();
    try {
      FuseDisparity(matcher, model, sources, motions, options, disp, nullptr, {}, &out);
      return 6;
    } catch (const std::invalid_argument& e) {
      std::printf("refused: %s\n", e.what());
    }
    std::printf("ok valid=%d kept=%d fused=%d filled=%d\n", counts[0], counts[1], counts[2], counts[3]);
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
