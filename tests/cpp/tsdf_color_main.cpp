// Drives the colour half of TsdfVolume of the C++ mirror (ocean-perception_amd/host/imaging.hpp) like a host caller.  Reads raw
// inputs written by tests/test_cpp_tsdf_color.py and writes raw outputs for it to compare with the definition
// (tests/tsdf_color_ref.py).
//   tsdf_color_main <dir> <rows> <cols> <n>   in: grid.f64 (nx, ny, nz, origin[3], voxel, trunc, max_weight), camera.f64 (fx, fy,
//                                             cx, cy, baseline), disp.f32 ([n][rows][cols]: n maps integrated from the identity
//                                             pose), bgr8.u8 ([n][rows][cols][3]: their images; the LAST frame goes in as floats,
//                                             value / 1), options.f32 (band, min_weight, byte_scale);  out: counts.i32 ([n][3]),
//                                             voxels.f32, colors.f32 (the two volumes), map.f32, map.u8 (ColorMap of the last
//                                             map), map_count.i32, xyz.f32, mesh_bgr.u8, tris.i32 (Mesh with colour), pts.f32,
//                                             pts_count.i32 (ColorPoints of the mesh's vertices), mesh.ply (WritePly of it)
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
    float o[3];
    std::vector<float> maps((size_t)n * px);
    std::vector<uint8_t> images((size_t)n * px * 3);
    if (!read_raw(dir + "/grid.f64", g, 9) || !read_raw(dir + "/camera.f64", c, 5) || !read_raw(dir + "/options.f32", o, 3) ||
        !read_raw(dir + "/disp.f32", maps.data(), maps.size()) || !read_raw(dir + "/bgr8.u8", images.data(), images.size())) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    TsdfGrid grid;
    grid.nx = (int)g[0], grid.ny = (int)g[1], grid.nz = (int)g[2];
    grid.origin = {{g[3], g[4], g[5]}};
    grid.voxel = g[6], grid.trunc = g[7], grid.max_weight = (float)g[8];
    StereoModel model;
    model.fx = c[0], model.fy = c[1], model.cx = c[2], model.cy = c[3], model.baseline = c[4];
    Motion identity;
    for (size_t i = 0; i < 9; ++i) identity.R[i] = i % 4 == 0 ? 1.0 : 0.0;
    for (size_t i = 0; i < 3; ++i) identity.t[i] = 0.0;
    bm::pm::PatchmatchGpu::Params params;
    params.max_rows = rows, params.max_cols = cols;
    bm::pm::PatchmatchGpu matcher(params);
    TsdfVolume plain(matcher, grid);  // the existing constructor: no colour volume
    if (plain.has_color() || plain.color_device()) return 7;
    try {
      plain.Mesh(TsdfMeshOptions(), true, /*want_color=*/true);
      return 6;
    } catch (const std::logic_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    TsdfVolume volume(matcher, grid, /*with_color=*/true);
    if (!volume.has_color() || !volume.color_device()) return 7;
    TsdfColorOptions options;
    options.band = o[0];
    std::vector<int> counts;
    bm::core::Image<float> disp(rows, cols);
    for (int k = 0; k < n; ++k) {
      std::copy(maps.begin() + (size_t)k * px, maps.begin() + (size_t)(k + 1) * px, disp.data());
      const uint8_t* const image = images.data() + (size_t)k * px * 3;
      std::array<int, 3> got;
      if (k + 1 < n) {
        bm::core::Image<bm::core::Vec3b> bgr(rows, cols);
        std::copy(image, image + 3 * px, reinterpret_cast<uint8_t*>(bgr.data()));
        got = volume.IntegrateColor(model, identity, disp, bgr, nullptr, options);
      } else {
        bm::core::Image<bm::core::Vec3f> bgr(rows, cols);
        for (size_t i = 0; i < 3 * px; ++i) reinterpret_cast<float*>(bgr.data())[i] = (float)image[i];
        got = volume.IntegrateColor(model, identity, disp, bgr, nullptr, options);
      }
      counts.insert(counts.end(), got.begin(), got.end());
    }
    write_raw(dir + "/counts.i32", counts.data(), counts.size());
    const std::vector<float> voxels = volume.Download();
    write_raw(dir + "/voxels.f32", voxels.data(), voxels.size());
    std::vector<float> colors(4 * volume.voxels());
    if (pm_download(matcher.handle(), colors.data(), volume.color_device(), sizeof(float) * colors.size()) != PM_OK) return 8;
    write_raw(dir + "/colors.f32", colors.data(), colors.size());
    TsdfColorSampleOptions sample;
    sample.min_weight = o[1], sample.byte_scale = o[2];
    bm::core::Image<bm::core::Vec3f> map;
    bm::core::Image<bm::core::Vec3b> map8;
    const int map_count = volume.ColorMap(model, identity, disp, &map, &map8, sample);
    write_raw(dir + "/map.f32", reinterpret_cast<const float*>(map.data()), 3 * px);
    write_raw(dir + "/map.u8", reinterpret_cast<const uint8_t*>(map8.data()), 3 * px);
    write_raw(dir + "/map_count.i32", &map_count, 1);
    const TriangleMesh mesh = volume.Mesh(TsdfMeshOptions(), /*want_normals=*/false, /*want_color=*/true, sample);
    const TriangleMesh grey = volume.Mesh();  // the existing call: normals, no colour
    if (mesh.vertices.bgr.size() != mesh.vertices.xyz.size() || !mesh.vertices.normals.empty() || !grey.vertices.bgr.empty() ||
        grey.vertices.normals.size() != mesh.vertices.xyz.size())
      return 7;
    write_raw(dir + "/xyz.f32", reinterpret_cast<const float*>(mesh.vertices.xyz.data()), 3 * mesh.vertices.xyz.size());
    write_raw(dir + "/mesh_bgr.u8", reinterpret_cast<const uint8_t*>(mesh.vertices.bgr.data()), 3 * mesh.vertices.bgr.size());
    write_raw(dir + "/tris.i32", reinterpret_cast<const int32_t*>(mesh.triangles.data()), 3 * mesh.triangles.size());
    std::vector<bm::core::Vec3f> pts;
    const int pts_count = volume.ColorPoints(mesh.vertices.xyz, &pts, nullptr, sample);
    write_raw(dir + "/pts.f32", reinterpret_cast<const float*>(pts.data()), 3 * pts.size());
    write_raw(dir + "/pts_count.i32", &pts_count, 1);
    WritePly(dir + "/mesh.ply", mesh);
    options.band = 0.f;
    try {
      volume.IntegrateColorDevice(model, identity, nullptr, nullptr, nullptr, nullptr, rows, cols, options);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    volume.Clear();
    if (volume.ColorMap(model, identity, disp, &map) != 0) return 9;  // Clear() clears the colour too
    std::printf("ok vertices=%d coloured=%d\n", (int)mesh.vertices.xyz.size(), pts_count);
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
