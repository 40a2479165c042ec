// tsdf_mesh_host_main.cpp -- runs the per-thread code of pm_tsdf_mesh (csrc/pm_tsdf_mesh_body.hpp: tsdf_mesh_flags_lane,
// tsdf_mesh_vertex_mask, tsdf_mesh_triangles_of, tsdf_mesh_vertices_lane, tsdf_mesh_triangles_lane and the case table -- the
// bodies of the kernels of csrc/pm_tsdf_mesh.hpp) on the HOST, so that tests/test_tsdf_mesh.py can hold it to the definition
// (tests/tsdf_mesh_ref.py) without a GPU and under -fsanitize=address,undefined.  The launches over whole volumes, a
// wavefront per span as the device forms them (host_launch.hpp's walk over the body header's kTsdfBlockX), spans and lanes
// forwards and then backwards: a slot may depend on the span offsets and the ranks alone, never on who ran first.  A lane's rank
// is the sum over the lanes below it, which is what the kernels' ballots compute.  Every buffer is a heap allocation of EXACTLY
// the bytes the stage may touch: the volume, the scratch of one byte and one word per node, two words per span and two per
// group of spans, and outputs of min(count, capacity) records.  Then once more with each output alone.
//   tsdf_mesh_host_main <dir>
// <dir> holds .npy dumps (host_npy.hpp: Case): params.npy (float64: nx, ny, nz, origin[3], voxel, trunc, max_weight, min_weight,
// vertex_capacity, tri_capacity), voxels.npy (float32 [nz][ny][nx][2]) and the definition's results want_counts.npy (int32 [2]:
// vertices, triangles), want_xyz.npy, want_normals.npy (float32 [min(vertices, vertex_capacity)][3]) and want_tris.npy (int32
// [min(triangles, tri_capacity)][3]).
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.

#include "host_launch.hpp"
#include "host_npy.hpp"
#include "pm_tsdf_mesh_body.hpp"

enum { kNx, kNy, kNz, kOrigin, kVoxel = kOrigin + 3, kTrunc, kMaxWeight, kMinWeight, kVertexCapacity, kTriCapacity, kParams };

// every span of a launch: body(span number, first node's i, j, k)
template <typename Body>
static void for_spans(const pm::TsdfMeshArgs& a, bool backwards, Body body) {
  for_blocks(a.x_spans, a.grid.ny, a.grid.nz, backwards, [&](int xs, int j, int k) {
    body(((size_t)k * a.grid.ny + j) * a.x_spans + xs, xs * pm::kTsdfLanes, j, k);
  });
}

// counts -> exclusive offsets in place, as k_cloud_offsets leaves them; returns the total
static int scan(int* counts, size_t n) {
  int total = 0;
  for (size_t i = 0; i < n; ++i) {
    const int c = counts[i];
    counts[i] = total;
    total += c;
  }
  return total;
}

// k_tsdf_mesh_span_offsets and k_cloud_offsets over one of the two: the spans' offsets inside their groups, the groups' sums
// scanned; returns the total
static int scan_spans(std::vector<int>& spans, std::vector<int>& groups, bool backwards) {
  for_blocks((long long)groups.size(), 1, 1, backwards, [&](int g, int, int) {
    const size_t first = (size_t)g * pm::kTsdfMeshGroup;
    const size_t n = spans.size() - first < (size_t)pm::kTsdfMeshGroup ? spans.size() - first : (size_t)pm::kTsdfMeshGroup;
    groups[g] = scan(spans.data() + first, n);
  });
  return scan(groups.data(), groups.size());
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Case c(argv[1]);
  const std::vector<double> p = c.params(kParams);
  pm_tsdf_volume vol = {};
  vol.nx = (int)p[kNx], vol.ny = (int)p[kNy], vol.nz = (int)p[kNz];
  for (int i = 0; i < 3; ++i) vol.origin[i] = p[kOrigin + i];
  vol.voxel = p[kVoxel], vol.trunc = p[kTrunc], vol.max_weight = (float)p[kMaxWeight];
  const int vcap = (int)p[kVertexCapacity], tcap = (int)p[kTriCapacity];
  if (c.failed || vol.nx < 1 || vol.ny < 1 || vol.nz < 1 || vcap < 0 || tcap < 0) return 2;
  const size_t nodes = (size_t)vol.nx * vol.ny * vol.nz;
  const auto voxels_b = c.raw("voxels", 8 * nodes);
  const auto want_counts = c.read<int32_t>("want_counts", 2);
  if (c.failed || want_counts[0] < 0 || want_counts[1] < 0) return 2;
  const size_t m = (size_t)(want_counts[0] < vcap ? want_counts[0] : vcap), t = (size_t)(want_counts[1] < tcap ? want_counts[1] : tcap);
  const auto want_xyz = c.raw("want_xyz", 12 * m), want_nrm = c.raw("want_normals", 12 * m), want_tris = c.raw("want_tris", 12 * t);
  if (c.failed) return 2;

  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const bool backwards = pass == 1;
    const char* const name = backwards ? "backwards" : "forwards";
    const auto voxels = exact_copy<pm::TsdfVoxel>(voxels_b.get(), nodes);
    pm::TsdfMeshArgs a = {};
    a.grid = pm::tsdf_grid(vol);
    a.min_weight = (float)p[kMinWeight];
    a.x_spans = (vol.nx + pm::kTsdfLanes - 1) / pm::kTsdfLanes;
    a.voxels = voxels.get();
    const size_t spans = (size_t)a.x_spans * vol.ny * vol.nz;
    std::unique_ptr<uint8_t[]> flags(new uint8_t[nodes]);
    std::unique_ptr<uint32_t[]> info(new uint32_t[nodes]);
    const size_t groups = (spans + pm::kTsdfMeshGroup - 1) / pm::kTsdfMeshGroup;
    std::vector<int> vertex_spans(spans), tri_spans(spans), vertex_groups(groups), tri_groups(groups);
    a.flags = flags.get(), a.info = info.get(), a.vertex_spans = vertex_spans.data(), a.tri_spans = tri_spans.data();
    a.vertex_groups = vertex_groups.data(), a.tri_groups = tri_groups.data();

    // k_tsdf_mesh_flags
    for_spans(a, backwards, [&](size_t, int i0, int j, int k) {
      for_threads(pm::kTsdfBlockX, 1, backwards, [&](int lane, int) {
        if (i0 + lane < vol.nx) a.flags[pm::tsdf_mesh_node(a.grid, i0 + lane, j, k)] = (uint8_t)pm::tsdf_mesh_flags_lane(a, i0 + lane, j, k);
      });
    });
    // k_tsdf_mesh_count: what each lane holds in front of the ballots, then the ranks
    for_spans(a, backwards, [&](size_t span, int i0, int j, int k) {
      unsigned mask[pm::kTsdfLanes] = {};
      int tris[pm::kTsdfLanes] = {};
      for_threads(pm::kTsdfBlockX, 1, backwards, [&](int lane, int) {
        if (i0 + lane >= vol.nx) return;
        const unsigned f = a.flags[pm::tsdf_mesh_node(a.grid, i0 + lane, j, k)];
        mask[lane] = pm::tsdf_mesh_vertex_mask(a, i0 + lane, j, k, f);
        tris[lane] = pm::tsdf_mesh_triangles_of(f);
      });
      int v_rank = 0, t_total = 0;
      for (int lane = 0; lane < pm::kTsdfLanes; ++lane) {
        if (i0 + lane < vol.nx) a.info[pm::tsdf_mesh_node(a.grid, i0 + lane, j, k)] = mask[lane] | ((uint32_t)v_rank << 8);
        v_rank += __builtin_popcount(mask[lane]);
        t_total += tris[lane];
      }
      a.vertex_spans[span] = v_rank, a.tri_spans[span] = t_total;
    });
    // k_tsdf_mesh_span_offsets, then k_cloud_offsets twice
    const int total[2] = {scan_spans(vertex_spans, vertex_groups, backwards), scan_spans(tri_spans, tri_groups, backwards)};
    if (total[0] != want_counts[0] || total[1] != want_counts[1]) {
      fprintf(stderr, "counts differ from the definition: %d vertices, %d triangles; it counts %d, %d (%s)\n", total[0], total[1],
              want_counts[0], want_counts[1], name);
      bad = 1;
      continue;
    }
    for (int outs = 7; outs >= 1; outs = outs == 7 ? 4 : outs >> 1) {  // all three, the triangles, the normals, the positions alone
      static const char* const which[8] = {"", "positions alone", "normals alone", "", "triangles alone", "", "", "every output"};
      const std::string label = std::string(name) + ", " + which[outs];
      std::unique_ptr<float[]> xyz, nrm;
      std::unique_ptr<int32_t[]> tris;
      if (outs & 1) xyz.reset(new float[3 * m ? 3 * m : 1]);
      if (outs & 2) nrm.reset(new float[3 * m ? 3 * m : 1]);
      if (outs & 4) tris.reset(new int32_t[3 * t ? 3 * t : 1]);
      a.xyz_out = xyz.get(), a.normals_out = nrm.get(), a.tri_out = tris.get();
      a.vertex_capacity = (outs & 3) ? vcap : 0, a.tri_capacity = (outs & 4) ? tcap : 0;
      // k_tsdf_mesh_vertices
      if (a.vertex_capacity > 0)
        for_spans(a, backwards, [&](size_t, int i0, int j, int k) {
          for_threads(pm::kTsdfBlockX, 1, backwards, [&](int lane, int) {
            if (i0 + lane < vol.nx) pm::tsdf_mesh_vertices_lane(a, i0 + lane, j, k);
          });
        });
      // k_tsdf_mesh_triangles
      if (a.tri_capacity > 0)
        for_spans(a, backwards, [&](size_t span, int i0, int j, int k) {
          int n[pm::kTsdfLanes] = {};
          for (int lane = 0; lane < pm::kTsdfLanes; ++lane)
            n[lane] = i0 + lane < vol.nx ? pm::tsdf_mesh_triangles_of(a.flags[pm::tsdf_mesh_node(a.grid, i0 + lane, j, k)]) : 0;
          for_threads(pm::kTsdfBlockX, 1, backwards, [&](int lane, int) {
            int rank = 0;
            for (int below = 0; below < lane; ++below) rank += n[below];
            if (n[lane]) pm::tsdf_mesh_triangles_lane(a, i0 + lane, j, k, pm::tsdf_mesh_tri_offset(a, span) + rank);
          });
        });
      if (outs & 1) bad |= differ("positions", xyz.get(), want_xyz.get(), 12 * m, label.c_str());
      if (outs & 2) bad |= differ("normals", nrm.get(), want_nrm.get(), 12 * m, label.c_str());
      if (outs & 4) bad |= differ("triangles", tris.get(), want_tris.get(), 12 * t, label.c_str());
    }
    bad |= differ("the volume behind the mesh", voxels.get(), voxels_b.get(), 8 * nodes, name);  // read only
  }
  return bad ? 1 : 0;
}
