// tsdf_host_main.cpp -- runs the per-thread code of pm_tsdf_integrate and pm_tsdf_raycast (csrc/pm_tsdf_body.hpp:
// tsdf_integrate_lane and tsdf_ray_lane, the bodies of k_tsdf_integrate and k_tsdf_raycast of csrc/pm_tsdf.hpp) on the HOST, so
// that tests/test_tsdf.py can hold it to the definition (tests/tsdf_ref.py) without a GPU and under
// -fsanitize=address,undefined.  Every buffer is a heap allocation of EXACTLY the bytes the stage may touch.  A sequence of
// integrates into one volume, then a raycast; all of it twice, spans / blocks and threads (host_launch.hpp's walk over the
// body header's kTsdfBlockX / Y) forwards and then backwards: the result must not depend on the order (no voxel and no pixel
// is touched by two threads, only integer addition crosses them).  The raycast then once more with each output alone and with
// the count alone.  Compiled as HIP source with the host-only switch of hipcc and -ffp-contract=off.
//   tsdf_host_main <dir>
// <dir> holds .npy dumps (host_npy.hpp: Case): params.npy (float64: nx, ny, nz, origin[3], voxel, trunc, max_weight, fx, fy,
// cx, cy, baseline, rows, cols, n (integrates, 1..4), min_disp, max_range, has_weight, the raycast's min_range, max_range,
// step, min_weight, its pose (R[9], t[3]), then 4 x the integrates' poses, the unused ones 0), start.npy (float32
// [nz][ny][nx][2]: the volume before the first integrate), disp.npy and weights.npy (float32 [n][rows][cols]; the weights are
// there and not read where has_weight is 0) and the definition's results want_voxels.npy (float32 [n][nz][ny][nx][2]: the
// volume behind each integrate), want_counts.npy (int32 [n][2]), want_disp.npy (float32 [rows][cols]), want_normals.npy
// (float32 [rows][cols][3]) and want_hits.npy (int32 [1]).
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.

#include "host_launch.hpp"
#include "host_npy.hpp"
#include "pm_tsdf_body.hpp"

static const int kMaxIntegrates = 4;
enum { kNx, kNy, kNz, kOrigin, kVoxel = kOrigin + 3, kTrunc, kMaxWeight, kFx, kFy, kCx, kCy, kBaseline, kRows, kCols, kN, kMinDisp,
       kMaxRange, kHasWeight, kRayMinRange, kRayMaxRange, kRayStep, kRayMinWeight, kRayPose, kPoses = kRayPose + 12,
       kParams = kPoses + 12 * kMaxIntegrates };

// every thread of every span of k_tsdf_integrate: a wavefront per span, the spans ceil(nx / 64) x ny x nz, x fastest
static void run_integrate(const pm::TsdfIntegrateArgs& a, bool backwards) {
  const pm::TsdfGrid& g = a.grid;
  for_blocks((g.nx + pm::kTsdfLanes - 1) / pm::kTsdfLanes, g.ny, g.nz, backwards, [&](int span, int j, int k) {
    int sums[2] = {0, 0};  // in view, updated
    for_threads(pm::kTsdfBlockX, 1, backwards, [&](int lane, int) {
      const int i = span * pm::kTsdfLanes + lane;
      add_flags<1>(i < g.nx ? pm::tsdf_integrate_lane(a, i, j, k) : 0u, sums);
    });
    flush_sums(a.counts, sums, pm::reproject_add);
  });
}

// every thread of every block of k_tsdf_raycast: grid (ceil(cols / 64), ceil(rows / 4))
static void run_raycast(const pm::TsdfRaycastArgs& a, bool backwards) {
  const int gx = (a.cols + pm::kTsdfBlockX - 1) / pm::kTsdfBlockX, gy = (a.rows + pm::kTsdfBlockY - 1) / pm::kTsdfBlockY;
  for_blocks(gx, gy, 1, backwards, [&](int bx, int by, int) {
    int sums[1] = {0};
    for_threads(pm::kTsdfBlockX, pm::kTsdfBlockY, backwards, [&](int tx, int ty) {
      const int x = bx * pm::kTsdfBlockX + tx, y = by * pm::kTsdfBlockY + ty;
      sums[0] += x < a.cols && y < a.rows && pm::tsdf_ray_lane(a, x, y) ? 1 : 0;
    });
    flush_sums(a.counts, sums, pm::reproject_add);
  });
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Case c(argv[1]);
  const std::vector<double> p = c.params(kParams);
  pm_tsdf_volume vol = {};
  vol.nx = (int)p[kNx], vol.ny = (int)p[kNy], vol.nz = (int)p[kNz];
  for (int i = 0; i < 3; ++i) vol.origin[i] = p[kOrigin + i];
  vol.voxel = p[kVoxel], vol.trunc = p[kTrunc], vol.max_weight = (float)p[kMaxWeight];
  const pm_cloud_camera camera = {p[kFx], p[kFy], p[kCx], p[kCy], p[kBaseline]};
  const int rows = (int)p[kRows], cols = (int)p[kCols], n = (int)p[kN];
  if (c.failed || vol.nx < 1 || vol.ny < 1 || vol.nz < 1 || rows < 1 || cols < 1 || n < 1 || n > kMaxIntegrates) return 2;
  const size_t vox = (size_t)vol.nx * vol.ny * vol.nz, px = (size_t)rows * cols;
  const auto start = c.raw("start", 8 * vox), disp_b = c.raw("disp", 4 * px * n), w_b = c.raw("weights", 4 * px * n);
  const auto want_vox = c.raw("want_voxels", 8 * vox * n), want_counts = c.raw("want_counts", 8 * (size_t)n);
  const auto want_disp = c.raw("want_disp", 4 * px), want_normals = c.raw("want_normals", 12 * px), want_hits = c.raw("want_hits", 4);
  if (c.failed) return 2;
  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const bool backwards = pass == 1;
    const char* const name = backwards ? "backwards" : "forwards";
    const auto voxels = exact_copy<pm::TsdfVoxel>(start.get(), vox);
    for (int k = 0; k < n; ++k) {
      std::unique_ptr<float[]> disp = exact_copy<float>(disp_b.get() + 4 * px * k, px), weight;
      if (p[kHasWeight] != 0.0) weight = exact_copy<float>(w_b.get() + 4 * px * k, px);
      int counts[2] = {0, 0};
      pm::TsdfIntegrateArgs a = {};
      a.cam = pm::cloud_cam(camera);
      a.grid = pm::tsdf_grid(vol);
      read_motion(&p[kPoses + 12 * k], a.R, a.t);
      a.min_disp = (float)p[kMinDisp], a.max_range = (float)p[kMaxRange];
      a.disp = disp.get(), a.weight = weight.get(), a.rows = rows, a.cols = cols;
      a.voxels = voxels.get(), a.counts = counts;
      run_integrate(a, backwards);
      const std::string what = "the volume behind integrate " + std::to_string(k);
      bad |= differ(what.c_str(), voxels.get(), want_vox.get() + 8 * vox * k, 8 * vox, name);
      bad |= differ("the integrate's counts", counts, want_counts.get() + 8 * k, 8, name);
      bad |= differ("the input map", disp.get(), disp_b.get() + 4 * px * k, 4 * px, name);  // read only
    }
    pm::TsdfRaycastArgs r = {};
    r.cam = pm::cloud_cam(camera);
    r.grid = pm::tsdf_grid(vol);
    double t[3];
    read_motion(&p[kRayPose], r.R, t);
    pm::motion_inverse(r.R, t, r.Ri, r.c);  // as pm_tsdf_raycast forms it on the host
    r.min_range = (double)(float)p[kRayMinRange], r.max_range = (double)(float)p[kRayMaxRange];
    r.ds = (double)(float)p[kRayStep] * vol.trunc;
    r.min_weight = (float)p[kRayMinWeight];
    r.n_samples = pm::tsdf_sample_count(r.min_range, r.max_range, r.ds);
    if (r.n_samples < 0) return 2;
    r.voxels = voxels.get(), r.rows = rows, r.cols = cols;
    for (int outs = 3; outs >= 0; --outs) {  // both outputs, the normals alone, the map alone, the count alone
      static const char* const which[4] = {"count alone", "map alone", "normals alone", "both outputs"};
      const std::string label = std::string(name) + ", " + which[outs];
      std::unique_ptr<float[]> disp_out, normals_out;
      if (outs & 1) disp_out.reset(new float[px]);
      if (outs & 2) normals_out.reset(new float[3 * px]);
      int hits = 0;
      r.disp_out = disp_out.get(), r.normals_out = normals_out.get(), r.counts = &hits;
      run_raycast(r, backwards);
      if (outs & 1) bad |= differ("disp", disp_out.get(), want_disp.get(), 4 * px, label.c_str());
      if (outs & 2) bad |= differ("normals", normals_out.get(), want_normals.get(), 12 * px, label.c_str());
      bad |= differ("hits", &hits, want_hits.get(), 4, label.c_str());
    }
    bad |= differ("the volume behind the raycast", voxels.get(), want_vox.get() + 8 * vox * (n - 1), 8 * vox, name);  // read only
  }
  return bad ? 1 : 0;
}
