// mesh_host_main.cpp -- runs pm_grid_mesh's own per-thread code (csrc/pm_mesh_body.hpp: mesh_value, mesh_cell,
// mesh_referenced, mesh_store_vertex, mesh_store_triangles -- the bodies of the kernels of csrc/pm_mesh.hpp) on the HOST, so
// that tests/test_mesh.py can hold it to the definition (tests/mesh_ref.py) without a GPU and under
// -fsanitize=address,undefined.  The blocks of the three launches are walked as the device forms them -- a block is `block`
// consecutive items of one grid row -- in forward or in reverse order: a slot may depend on the block offsets alone, never
// on which block ran first (host_launch.hpp's block walk).  Every buffer is a heap allocation of EXACTLY the bytes the stage
// may touch: a load past the last disparity or slot-map entry, or a store behind slot min(count, capacity) - 1, is reported.
// Compiled as HIP source with the host-only switch of hipcc and -ffp-contract=off.
//   mesh_host_main <dir>
// <dir> holds .npy dumps (host_npy.hpp: Case): params.npy (float64: rows, cols, fx, fy, cx, cy, baseline, min_disp, max_range,
// stride, max_diff, vertices, vertex_capacity, tri_capacity, block, reverse), disp.npy (float32 [rows][cols]), normals.npy
// (float32 [rows][cols][3]), bgr.npy (uint8 [rows][cols][3]) and the definition's results want_counts.npy (int32 [2]:
// vertices, triangles), want_xyz.npy, want_normals.npy, want_bgr.npy, want_index.npy (min(vertices, vertex_capacity) entries
// each) and want_tris.npy (int32 [min(triangles, tri_capacity)][3]).
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.

#include "host_launch.hpp"
#include "host_npy.hpp"
#include "pm_mesh_body.hpp"

enum { kRows, kCols, kFx, kFy, kCx, kCy, kBaseline, kMinDisp, kMaxRange, kStride, kMaxDiff, kVertices, kVertexCapacity, kTriCapacity,
       kBlock, kReverse, kParams };

// what a thread of block (ys, xs0 + k) computes in the count and in the scatter launches
static bool thread_vertex(const pm::MeshArgs& a, int xs, int ys) {
  if (!a.referenced) return pm::mesh_value(a, xs, ys) > 0.f;
  float v[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) v[r][c] = pm::mesh_value(a, xs - 1 + c, ys - 1 + r);
  return pm::mesh_referenced(v, a.max_diff);
}
static unsigned thread_cell(const pm::MeshArgs& a, int xs, int ys) {
  return pm::mesh_cell(pm::mesh_value(a, xs, ys), pm::mesh_value(a, xs + 1, ys), pm::mesh_value(a, xs, ys + 1),
                       pm::mesh_value(a, xs + 1, ys + 1), a.max_diff);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Case c(argv[1]);
  const std::vector<double> p = c.params(kParams);
  const int rows = (int)p[kRows], cols = (int)p[kCols], stride = (int)p[kStride], vertices = (int)p[kVertices],
            vcap = (int)p[kVertexCapacity], tcap = (int)p[kTriCapacity], block = (int)p[kBlock], reverse = (int)p[kReverse];
  const pm_cloud_camera camera = {p[kFx], p[kFy], p[kCx], p[kCy], p[kBaseline]};
  const pm_cloud_filter filter = {(float)p[kMinDisp], (float)p[kMaxRange], stride};
  if (c.failed || rows < 1 || cols < 1 || stride < 1 || vcap < 0 || tcap < 0 || block < 1 || (vertices != 0 && vertices != 1)) return 2;
  const size_t px = (size_t)rows * cols;
  const auto disp = c.read<float>("disp", px), normals = c.read<float>("normals", 3 * px);
  const auto bgr_b = c.raw("bgr", 3 * px);
  const auto want_counts = c.read<int32_t>("want_counts", 2);
  if (c.failed || want_counts[0] < 0 || want_counts[1] < 0) return 2;
  const int32_t* const want_n = want_counts.get();
  const size_t m = (size_t)(want_n[0] < vcap ? want_n[0] : vcap), t = (size_t)(want_n[1] < tcap ? want_n[1] : tcap);
  const auto want_xyz = c.raw("want_xyz", 12 * m), want_nrm = c.raw("want_normals", 12 * m), want_bgr = c.raw("want_bgr", 3 * m);
  const auto want_idx = c.raw("want_index", 4 * m), want_tris = c.raw("want_tris", 12 * t);
  if (c.failed) return 2;

  const int sub_rows = pm::cloud_grid(rows, stride);
  const pm::MeshArgs a = {pm::cloud_args(camera, filter, disp.get(), rows, cols), sub_rows, (float)p[kMaxDiff], vertices};
  const int sub_cols = a.c.sub_cols;
  const int segments = (sub_cols + block - 1) / block, blocks = sub_rows * segments;

  // the count launch, then the two scans
  std::vector<int> voff(blocks), toff(blocks);
  for_blocks(segments, sub_rows, 1, reverse, [&](int segment, int ys, int) {
    const int b = ys * segments + segment, xs0 = segment * block;
    int nv = 0, nt = 0;
    for (int k = 0; k < block; ++k) {
      nv += thread_vertex(a, xs0 + k, ys);
      const unsigned cell = thread_cell(a, xs0 + k, ys);
      nt += (int)(cell & pm::kMeshT0) + (int)((cell & pm::kMeshT1) != 0);
    }
    voff[b] = nv, toff[b] = nt;
  });
  int total[2] = {0, 0};
  for (int b = 0; b < blocks; ++b) {
    const int nv = voff[b], nt = toff[b];
    voff[b] = total[0], toff[b] = total[1];
    total[0] += nv, total[1] += nt;
  }
  int bad = 0;
  if (total[0] != want_n[0] || total[1] != want_n[1]) {
    fprintf(stderr, "counts %d vertices, %d triangles; the definition counts %d, %d\n", total[0], total[1], want_n[0], want_n[1]);
    bad = 1;
  }

  // the vertex scatter: streams of exactly min(count, capacity) records, a slot map of exactly the grid
  std::unique_ptr<float[]> xyz(new float[3 * m ? 3 * m : 1]), nrm(new float[3 * m ? 3 * m : 1]);
  std::unique_ptr<uint8_t[]> bgr(new uint8_t[3 * m ? 3 * m : 1]);
  std::unique_ptr<int32_t[]> idx(new int32_t[m ? m : 1]), tris(new int32_t[3 * t ? 3 * t : 1]);
  std::unique_ptr<int32_t[]> slot_map(new int32_t[(size_t)a.c.items]);
  const pm::CloudStreams cs = {normals.get(), bgr_b.get(), xyz.get(), nrm.get(), bgr.get(), idx.get(), vcap};
  for_blocks(segments, sub_rows, 1, reverse, [&](int segment, int ys, int) {
    const int xs0 = segment * block;
    int slot = voff[ys * segments + segment];
    for (int k = 0; k < block; ++k) {
      const bool is_vertex = thread_vertex(a, xs0 + k, ys);
      if (xs0 + k < sub_cols) pm::mesh_store_vertex(a, cs, slot_map.get(), xs0 + k, ys, is_vertex, slot);
      slot += is_vertex;
    }
  });
  // the triangle scatter
  for_blocks(segments, sub_rows, 1, reverse, [&](int segment, int ys, int) {
    const int xs0 = segment * block;
    int slot = toff[ys * segments + segment];
    for (int k = 0; k < block; ++k) {
      const unsigned cell = thread_cell(a, xs0 + k, ys);
      if (cell & (pm::kMeshT0 | pm::kMeshT1)) pm::mesh_store_triangles(a, slot_map.get(), tris.get(), tcap, xs0 + k, ys, cell, slot);
      slot += (int)(cell & pm::kMeshT0) + (int)((cell & pm::kMeshT1) != 0);
    }
  });
  bad |= differ("mesh xyz", xyz.get(), want_xyz.get(), 12 * m);
  bad |= differ("mesh normals", nrm.get(), want_nrm.get(), 12 * m);
  bad |= differ("mesh bgr", bgr.get(), want_bgr.get(), 3 * m);
  bad |= differ("mesh index", idx.get(), want_idx.get(), 4 * m);
  bad |= differ("mesh triangles", tris.get(), want_tris.get(), 12 * t);
  return bad ? 1 : 0;
}
