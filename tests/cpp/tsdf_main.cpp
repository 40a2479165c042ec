// Drives TsdfVolume of the C++ mirror (ocean-perception_amd/host/imaging.hpp) like a host caller.  Reads raw inputs written by
// tests/test_cpp_tsdf.py and writes raw outputs for it to compare with the definition (tests/tsdf_ref.py).
//   tsdf_main <dir> <rows> <cols> <n>   in: grid.f64 (nx, ny, nz, origin[3], voxel, trunc, max_weight), camera.f64 (fx, fy, cx,
//                                       cy, baseline), disp.f32 ([n][rows][cols]), weights.f32 ([rows][cols], for map 0; the
//                                       others have none), poses.f64 ((n + 1) x (R[9], t[3]): the integrates', then the
//                                       raycast's), ray.f32 (min_range, max_range, step, min_weight);  out: volume.f32 (behind
//                                       the n integrates), counts.i32 ([n][2]), disp_out.f32, normals.f32, hits.i32 ([2]: of the
//                                       call with both outputs and of a call that asks for the map alone), map_only.f32, and
//                                       cleared.f32: the volume behind Clear()
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
    const size_t px = (size_t)rows * cols;
    double g[9], c[5];
    float r[4];
    std::vector<float> maps((size_t)n * px);
    std::vector<double> pv((size_t)(n + 1) * 12);
    bm::core::Image<float> weight(rows, cols);
    if (!read_raw(dir + "/grid.f64", g, 9) || !read_raw(dir + "/camera.f64", c, 5) || !read_raw(dir + "/ray.f32", r, 4) ||
        !read_raw(dir + "/disp.f32", maps.data(), maps.size()) || !read_raw(dir + "/poses.f64", pv.data(), pv.size()) ||
        !read_raw(dir + "/weights.f32", weight)) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    TsdfGrid grid;
    grid.nx = (int)g[0], grid.ny = (int)g[1], grid.nz = (int)g[2];
    grid.origin = {{g[3], g[4], g[5]}};
    grid.voxel = g[6], grid.trunc = g[7], grid.max_weight = (float)g[8];
    StereoModel model;
    model.fx = c[0], model.fy = c[1], model.cx = c[2], model.cy = c[3], model.baseline = c[4];
    std::vector<Motion> poses((size_t)n + 1);
    for (size_t k = 0; k < poses.size(); ++k) {
      for (size_t i = 0; i < 9; ++i) poses[k].R[i] = pv[k * 12 + i];
      for (size_t i = 0; i < 3; ++i) poses[k].t[i] = pv[k * 12 + 9 + i];
    }
    bm::pm::PatchmatchGpu unplanned{bm::pm::PatchmatchGpu::Params()};
    try {
      TsdfVolume none(unplanned, grid);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    bm::pm::PatchmatchGpu::Params params;
    params.max_rows = rows, params.max_cols = cols;
    bm::pm::PatchmatchGpu matcher(params);
    TsdfGrid bad = grid;
    bad.voxel = 0.0;
    try {
      TsdfVolume none(matcher, bad);
      return 6;
    } catch (const std::invalid_argument& e) {
      std::printf("refused: %s\n", e.what());
    }
    TsdfVolume volume(matcher, grid);
    std::vector<int> counts;
    for (int k = 0; k < n; ++k) {
      bm::core::Image<float> disp(rows, cols);
      std::copy(maps.begin() + (size_t)k * px, maps.begin() + (size_t)(k + 1) * px, disp.data());
      const std::array<int, 2> got = volume.Integrate(model, poses[(size_t)k], disp, k == 0 ? &weight : nullptr);
      counts.push_back(got[0]);
      counts.push_back(got[1]);
    }
    const std::vector<float> records = volume.Download();
    write_raw(dir + "/volume.f32", records.data(), records.size());
    write_raw(dir + "/counts.i32", counts.data(), counts.size());
    TsdfRaycastOptions ray;
    ray.min_range = r[0], ray.max_range = r[1], ray.step = r[2], ray.min_weight = r[3];
    bm::core::Image<float> out, map_only;
    bm::core::Image<bm::core::Vec3f> normals;
    int hits[2];
    hits[0] = volume.Raycast(model, poses[(size_t)n], rows, cols, &out, &normals, ray);
    hits[1] = volume.Raycast(model, poses[(size_t)n], rows, cols, &map_only, nullptr, ray);
    write_raw(dir + "/disp_out.f32", out);
    write_raw(dir + "/normals.f32", reinterpret_cast<const float*>(normals.data()), 3 * px);
    write_raw(dir + "/map_only.f32", map_only);
    write_raw(dir + "/hits.i32", hits, 2);
    ray.step = 1.5f;
    try {
      volume.Raycast(model, poses[(size_t)n], rows, cols, &out, nullptr, ray);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    bm::core::Image<float> other(rows + 1, cols);
    try {
      bm::core::Image<float> disp(rows, cols);
      volume.Integrate(model, poses[0], disp, &other);
      return 6;
    } catch (const std::invalid_argument& e) {
      std::printf("refused: %s\n", e.what());
    }
    volume.Clear();
    const std::vector<float> cleared = volume.Download();
    write_raw(dir + "/cleared.f32", cleared.data(), cleared.size());
    std::printf("ok in_view=%d updated=%d hit=%d\n", counts[0], counts[1], hits[0]);
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
