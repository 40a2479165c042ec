// Drives the mesh functions of the C++ mirror (ocean-perception_amd/host/imaging.hpp: MakeGridMesh, WritePly) like a host
// caller.  Reads raw inputs written by tests/test_cpp_mesh.py and writes raw outputs for it to compare with the definition
// (tests/mesh_ref.py).
//   mesh_main ply <dir>                 no device: a hand-made mesh of four vertices and two triangles through WritePly as
//                                       plain.ply (points alone), normals.ply and full.ply (normals and colour)
//   mesh_main mesh <dir> <rows> <cols>  in: disp.f32, normals.f32, bgr.u8 (a map, organised normals and a colour image)
//                                       out: ref_{xyz.f32, normals.f32, bgr.u8, index.i32, tris.i32}: REFERENCED vertices,
//                                       min_disp 8.5, stride 2, max_diff 0.5, with normals and colour, and ref.ply of it;
//                                       all_{xyz.f32, index.i32, tris.i32}: every vertex, stride 1, nothing else
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "imaging.hpp"
#include "raw_io.hpp"

using namespace bm::imaging;

static int ply_only(const std::string& dir) {
  TriangleMesh mesh;
  for (int k = 0; k < 4; ++k) {
    mesh.vertices.xyz.push_back(bm::core::Vec3f{{0.5f * (float)(k & 1), -0.25f * (float)(k >> 1), 1.f + (float)k}});
    mesh.vertices.index.push_back(k);
  }
  mesh.triangles.push_back({0, 2, 3});
  mesh.triangles.push_back({0, 3, 1});
  WritePly(dir + "/plain.ply", mesh);
  for (int k = 0; k < 4; ++k) mesh.vertices.normals.push_back(bm::core::Vec3f{{0.f, 0.125f * (float)k, -1.f}});
  WritePly(dir + "/normals.ply", mesh);
  for (int k = 0; k < 4; ++k) mesh.vertices.bgr.push_back(bm::core::Vec3b{{(uint8_t)(10 + k), (uint8_t)(20 + k), (uint8_t)(30 + k)}});
  WritePly(dir + "/full.ply", mesh);
  WritePly(dir + "/empty.ply", TriangleMesh());
  try {
    WritePly(dir + "/no/such/directory/x.ply", mesh);
    return 7;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  std::printf("ok ply\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string what = argv[1], dir = argv[2];
  try {
    if (what == "ply") return ply_only(dir);
    if (what != "mesh" || argc < 5) return 2;
    const int rows = atoi(argv[3]), cols = atoi(argv[4]);
    bm::core::Image<float> disp(rows, cols);
    bm::core::Image<bm::core::Vec3f> normals(rows, cols);
    bm::core::Image<bm::core::Vec3b> bgr(rows, cols);
    if (!read_raw(dir + "/disp.f32", disp) || !read_raw(dir + "/normals.f32", normals) || !read_raw(dir + "/bgr.u8", bgr)) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    StereoModel model;
    model.fx = 412.7, model.fy = 398.3, model.cx = cols / 2 - 0.3, model.cy = rows / 2 + 0.4, model.baseline = 0.12;
    CloudFilter filter;
    filter.min_disp = 8.5f;
    filter.stride = 2;
    MeshOptions options;
    options.max_diff = 0.5f;
    const TriangleMesh ref = MakeGridMesh(disp, model, filter, options, &normals, &bgr);
    const PointCloud& v = ref.vertices;
    if (v.normals.size() != v.xyz.size() || v.bgr.size() != v.xyz.size() || v.index.size() != v.xyz.size()) return 4;
    write_raw(dir + "/ref_xyz.f32", v.xyz.data(), v.xyz.size());
    write_raw(dir + "/ref_normals.f32", v.normals.data(), v.normals.size());
    write_raw(dir + "/ref_bgr.u8", v.bgr.data(), v.bgr.size());
    write_raw(dir + "/ref_index.i32", v.index.data(), v.index.size());
    write_raw(dir + "/ref_tris.i32", ref.triangles.data(), ref.triangles.size());
    WritePly(dir + "/ref.ply", ref);
    options.referenced_vertices = false;
    const TriangleMesh all = MakeGridMesh(disp, model, CloudFilter(), options);
    if (!all.vertices.normals.empty() || !all.vertices.bgr.empty()) return 4;
    write_raw(dir + "/all_xyz.f32", all.vertices.xyz.data(), all.vertices.xyz.size());
    write_raw(dir + "/all_index.i32", all.vertices.index.data(), all.vertices.index.size());
    write_raw(dir + "/all_tris.i32", all.triangles.data(), all.triangles.size());
    // a map without a counting pixel: an empty mesh, not an error
    bm::core::Image<float> none(rows, cols);
    for (size_t i = 0; i < (size_t)rows * cols; ++i) none.data()[i] = 0.f;
    const TriangleMesh empty = MakeGridMesh(none, model);
    if (!empty.vertices.xyz.empty() || !empty.triangles.empty()) return 5;
    options.max_diff = -1.f;
    try {
      MakeGridMesh(disp, model, filter, options);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    std::printf("ok vertices=%zu triangles=%zu all_vertices=%zu all_triangles=%zu\n", v.xyz.size(), ref.triangles.size(),
                all.vertices.xyz.size(), all.triangles.size());
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
