// Drives the temporal-seed functions of the C++ mirror (ocean-perception_amd/host/imaging.hpp: RelativeMotion,
// ReprojectDisparity) like a host caller.  Reads raw inputs written by tests/test_cpp_reproject.py and writes raw outputs
// for it to compare with the definition (tests/reproject_ref.py).
//   reproject_main motion <dir>                    no device: poses.f64 (T_world_old, T_world_new: 2 x 16 doubles) ->
//                                                  motion.f64 (R[9], t[3])
//   reproject_main reproject <dir> <rows> <cols>   in: disp.f32 (the old left map), motion.f64;  out: seed_l.f32, seed_r.f32,
//                                                  counts.i32 (min_disp 1, close_radius 2), and right_only.f32 /
//                                                  right_only_counts.i32 of a call without d_seed_l that only enqueues
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "imaging.hpp"
#include "raw_io.hpp"

using namespace bm::imaging;

// device memory of the matcher's handle, freed on scope exit
struct Device {
  pm_handle* h;
  void* p = nullptr;
  Device(pm_handle* handle, size_t bytes) : h(handle) {
    if (pm_device_malloc(h, bytes, &p) != PM_OK) throw std::runtime_error("pm_device_malloc failed");
  }
  ~Device() { pm_device_free(h, p); }
  Device(const Device&) = delete;
  Device& operator=(const Device&) = delete;
  float* f() { return static_cast<float*>(p); }
};

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string what = argv[1], dir = argv[2];
  try {
    if (what == "motion") {
      double poses[32];
      if (!read_raw(dir + "/poses.f64", poses, 32)) return 3;
      const Motion m = RelativeMotion(poses, poses + 16);
      double out[12];
      for (size_t i = 0; i < 9; ++i) out[i] = m.R[i];
      for (size_t i = 0; i < 3; ++i) out[9 + i] = m.t[i];
      write_raw(dir + "/motion.f64", out, 12);
      const Motion same = RelativeMotion(poses, poses);  // a camera that did not move
      const Motion none;
      for (size_t i = 0; i < 9; ++i)
        if (std::abs(same.R[i] - none.R[i]) > 1e-15) return 4;
      for (size_t i = 0; i < 3; ++i)
        if (same.t[i] != 0.0) return 4;
      std::printf("ok motion\n");
      return 0;
    }
    if (what != "reproject" || argc < 5) return 2;
    const int rows = atoi(argv[3]), cols = atoi(argv[4]);
    const size_t px = (size_t)rows * cols;
    std::vector<float> disp(px), seed_l(px), seed_r(px), right_only(px);
    double mv[12];
    if (!read_raw(dir + "/disp.f32", disp.data(), px) || !read_raw(dir + "/motion.f64", mv, 12)) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    Motion motion;
    for (size_t i = 0; i < 9; ++i) motion.R[i] = mv[i];
    for (size_t i = 0; i < 3; ++i) motion.t[i] = mv[9 + i];
    StereoModel model;
    model.fx = 412.7, model.fy = 398.3, model.cx = cols / 2 - 0.3, model.cy = rows / 2 + 0.4, model.baseline = 0.12;
    bm::pm::PatchmatchGpu::Params params;
    params.max_rows = rows, params.max_cols = cols;
    bm::pm::PatchmatchGpu unplanned{bm::pm::PatchmatchGpu::Params()};
    try {
      ReprojectDisparity(unplanned, model, motion, nullptr, rows, cols, nullptr, nullptr);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    bm::pm::PatchmatchGpu matcher(params);
    pm_handle* h = matcher.handle();
    Device d_disp(h, 4 * px), d_l(h, 4 * px), d_r(h, 4 * px);
    if (pm_upload(h, d_disp.p, disp.data(), 4 * px) != PM_OK) return 5;
    ReprojectOptions options;
    options.min_disp = 1.f;
    options.close_radius = 2;
    const std::array<int, 2> counts = ReprojectDisparity(matcher, model, motion, d_disp.f(), rows, cols, d_l.f(), d_r.f(), options);
    if (pm_download(h, seed_l.data(), d_l.p, 4 * px) != PM_OK || pm_download(h, seed_r.data(), d_r.p, 4 * px) != PM_OK) return 5;
    write_raw(dir + "/seed_l.f32", seed_l.data(), px);
    write_raw(dir + "/seed_r.f32", seed_r.data(), px);
    write_raw(dir + "/counts.i32", counts.data(), 2);
    // the right seed alone, without waiting for the counts: the download is ordered behind it on the handle's stream
    const std::array<int, 2> none = ReprojectDisparity(matcher, model, motion, d_disp.f(), rows, cols, nullptr, d_r.f(), options, false);
    if (pm_download(h, right_only.data(), d_r.p, 4 * px) != PM_OK) return 5;
    write_raw(dir + "/right_only.f32", right_only.data(), px);
    write_raw(dir + "/right_only_counts.i32", none.data(), 2);
    options.close_radius = 4;
    try {
      ReprojectDisparity(matcher, model, motion, d_disp.f(), rows, cols, d_l.f(), d_r.f(), options);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    std::printf("ok seeds_l=%d seeds_r=%d\n", counts[0], counts[1]);
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
