// Drives TrackFeatures, SolveMotion and EstimateMotion of the C++ mirror (ocean-perception_amd/host/imaging.hpp) like a host
// caller.  Reads raw inputs written by tests/test_cpp_motion.py and writes raw outputs for it to compare with the definition
// (tests/motion_ref.py) and with the C ABI.
//   motion_caller_main <dir> <rows> <cols>   in: old.u8, new.u8 (the two left images), disp.f32 (the old left map);
//                                            out: tracks.bin (32-byte records), solved.f64 (R[9], t[3] of SolveMotion on
//                                            them), solved_info.i32 / solved_rms.f64, estimated.f64, estimated_info.i32 /
//                                            estimated_rms.f64 (EstimateMotion), with cell 8, patch_radius 5, search_radius
//                                            20, 20 iterations, epsilon 1e-10, min_inliers 30, from the identity guess
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "imaging.hpp"
#include "raw_io.hpp"

using namespace bm::imaging;

static void write_motion(const std::string& stem, const Motion& m, const pm_motion_info& info) {
  double v[12];
  for (size_t i = 0; i < 9; ++i) v[i] = m.R[i];
  for (size_t i = 0; i < 3; ++i) v[9 + i] = m.t[i];
  const int n[5] = {info.valid, info.n_tracks, info.n_used, info.n_inliers, info.iterations};
  write_raw(stem + ".f64", v, 12);
  write_raw(stem + "_info.i32", n, 5);
  write_raw(stem + "_rms.f64", &info.rms_px, 1);
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::string dir = argv[1];
  const int rows = atoi(argv[2]), cols = atoi(argv[3]);
  if (rows < 1 || cols < 1) return 2;
  try {
    bm::core::Image<uint8_t> old(rows, cols), img(rows, cols);
    bm::core::Image<float> disp(rows, cols);
    if (!read_raw(dir + "/old.u8", old) || !read_raw(dir + "/new.u8", img) || !read_raw(dir + "/disp.f32", disp)) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    StereoModel model;
    model.fx = 412.7, model.fy = 398.3, model.cx = cols / 2 - 0.3, model.cy = rows / 2 + 0.4, model.baseline = 0.12;
    TrackOptions track;
    track.cell = 8, track.patch_radius = 5, track.search_radius = 20;
    SolveOptions solve;
    solve.iterations = 20, solve.epsilon = 1e-10, solve.min_inliers = 30;
    bm::pm::PatchmatchGpu unplanned{bm::pm::PatchmatchGpu::Params()};
    try {
      TrackFeatures(unplanned, model, track, nullptr, old, disp, img);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    bm::pm::PatchmatchGpu::Params params;
    params.max_rows = rows, params.max_cols = cols;
    bm::pm::PatchmatchGpu matcher(params);
    const std::vector<pm_track> tracks = TrackFeatures(matcher, model, track, nullptr, old, disp, img);
    write_raw(dir + "/tracks.bin", tracks.data(), tracks.size());
    pm_motion_info info;
    const Motion solved = SolveMotion(model, solve, tracks, nullptr, &info);
    write_motion(dir + "/solved", solved, info);
    const Motion estimated = EstimateMotion(matcher, model, track, solve, nullptr, old, disp, img, &info);
    write_motion(dir + "/estimated", estimated, info);
    track.search_radius = 25;
    try {
      EstimateMotion(matcher, model, track, solve, nullptr, old, disp, img);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    track.search_radius = 20;
    solve.min_inliers = 5;
    try {
      SolveMotion(model, solve, tracks, nullptr);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    bm::core::Image<float> small(rows - 1, cols);
    try {
      TrackFeatures(matcher, model, track, nullptr, old, small, img);
      return 6;
    } catch (const std::invalid_argument& e) {
      std::printf("refused: %s\n", e.what());
    }
    std::printf("ok tracks=%zu valid=%d inliers=%d\n", tracks.size(), info.valid, info.n_inliers);
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
