// Drives the point-cloud functions of the C++ mirror (ocean-perception_amd/host/imaging.hpp: Backproject, MakePointCloud,
// PlaneNormals) like a host caller: host images in, host images / vectors out.  Reads raw inputs written by
// tests/test_cpp_pointcloud.py and writes raw outputs for it to compare with the C ABI calls and the definition.
//   pointcloud_main <dir> <rows> <cols>
// in:  disp.f32, bgr.u8 (a map and a colour image of one size), left.u8, right.u8 (a rectified pair)
// out: xyz.f32; cloud_{xyz.f32, bgr.u8, index.i32} (min_disp 5, stride 2, with colour); and from a PM_MODE_PLANES Match()
//      of the pair: match_l.f32, planes.f32 (pm_planes_read of the left view), normals.f32 (masked by match_l),
//      ncloud_{xyz.f32, normals.f32, index.i32} (the match's cloud with normals)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

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
    bm::core::Image<bm::core::Vec3b> bgr(rows, cols);
    bm::core::Image<uint8_t> left(rows, cols), right(rows, cols);
    if (!read_raw(dir + "/disp.f32", disp) || !read_raw(dir + "/bgr.u8", bgr) || !read_raw(dir + "/left.u8", left) ||
        !read_raw(dir + "/right.u8", right)) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    StereoModel model;
    model.fx = 412.7, model.fy = 398.3, model.cx = cols / 2 - 0.3, model.cy = rows / 2 + 0.4, model.baseline = 0.12;
    const bm::core::Image<bm::core::Vec3f> xyz = Backproject(disp, model);
    write_raw(dir + "/xyz.f32", xyz.data(), px);
    CloudFilter filter;
    filter.min_disp = 5.0f;
    filter.stride = 2;
    const PointCloud pc = MakePointCloud(disp, model, filter, nullptr, &bgr);
    if (!pc.normals.empty() || pc.bgr.size() != pc.xyz.size() || pc.index.size() != pc.xyz.size()) return 4;
    write_raw(dir + "/cloud_xyz.f32", pc.xyz.data(), pc.xyz.size());
    write_raw(dir + "/cloud_bgr.u8", pc.bgr.data(), pc.bgr.size());
    write_raw(dir + "/cloud_index.i32", pc.index.data(), pc.index.size());

    bm::pm::PatchmatchGpu::Params params;
    params.semantics = PM_SEM_CPU;
    params.mode = PM_MODE_PLANES;
    params.patch_size = 7;
    params.patchmatch_iters = 2;
    bm::pm::PatchmatchGpu matcher(params);
    bm::core::Image<float> match_l, match_r;
    matcher.Match(left, right, match_l, match_r);
    write_raw(dir + "/match_l.f32", match_l.data(), px);
    std::vector<float> planes(4 * px);
    if (pm_planes_read(matcher.handle(), 0, 0, planes.data()) != PM_OK) return 5;
    write_raw(dir + "/planes.f32", planes.data(), planes.size());
    const bm::core::Image<bm::core::Vec3f> normals = PlaneNormals(matcher, model, rows, cols, &match_l);
    write_raw(dir + "/normals.f32", normals.data(), px);
    const PointCloud nc = MakePointCloud(match_l, model, CloudFilter(), &normals, nullptr);
    if (!nc.bgr.empty() || nc.normals.size() != nc.xyz.size()) return 4;
    write_raw(dir + "/ncloud_xyz.f32", nc.xyz.data(), nc.xyz.size());
    write_raw(dir + "/ncloud_normals.f32", nc.normals.data(), nc.normals.size());
    write_raw(dir + "/ncloud_index.i32", nc.index.data(), nc.index.size());
    // a scalar-mode matcher keeps no slopes: refused, not approximated
    bm::pm::PatchmatchGpu::Params scalar;
    scalar.semantics = PM_SEM_CPU;
    scalar.patch_size = 7;
    bm::pm::PatchmatchGpu plain(scalar);
    plain.Match(left, right, match_l, match_r);
    try {
      PlaneNormals(plain, model, rows, cols);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    std::printf("ok points=%zu match_points=%zu\n", pc.xyz.size(), nc.xyz.size());
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
