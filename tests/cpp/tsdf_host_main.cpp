// tsdf_host_main.cpp -- runs the per-thread code of pm_tsdf_integrate and pm_tsdf_raycast (csrc/pm_tsdf_body.hpp:
// tsdf_integrate_lane and tsdf_ray_lane, the bodies of k_tsdf_integrate and k_tsdf_raycast of csrc/pm_tsdf.hpp) on the HOST, so
// that tests/test_tsdf.py can hold it to the definition (tests/tsdf_ref.py) without a GPU and under
// -fsanitize=address,undefined.  Every buffer is a heap allocation of EXACTLY the bytes the stage may touch.  A sequence of
// integrates into one volume, then a raycast; all of it twice, spans / blocks and threads forwards and then backwards: the
// result must not depend on the order (no voxel and no pixel is touched by two threads, only integer addition crosses them).
// The raycast then once more with each output alone and with the count alone.  Compiled as HIP source with the host-only switch
// of hipcc and -ffp-contract=off.
//   tsdf_host_main <dir>
// <dir> holds .npy dumps (numpy's format, version 1, C order, little endian): params.npy (float64: nx, ny, nz, origin[3], voxel,
// trunc, max_weight, fx, fy, cx, cy, baseline, rows, cols, n (integrates, 1..4), min_disp, max_range, has_weight, the raycast's
// min_range, max_range, step, min_weight, its pose (R[9], t[3]), then 4 x the integrates' poses, the unused ones 0), start.npy
// (float32 [nz][ny][nx][2]: the volume before the first integrate), disp.npy and weights.npy (float32 [n][rows][cols]; the
// weights are there and not read where has_weight is 0) and the definition's results want_voxels.npy (float32
// [n][nz][ny][nx][2]: the volume behind each integrate), want_counts.npy (int32 [n][2]), want_disp.npy (float32 [rows][cols]),
// want_normals.npy (float32 [rows][cols][3]) and want_hits.npy (int32 [1]).
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "host_npy.hpp"
#include "pm_tsdf_body.hpp"

static const int kMaxIntegrates = 4;
static const int kHead = 24;
static const int kParams = kHead + 12 + 12 * kMaxIntegrates;

static long long nth(long long i, long long n, bool backwards) { return backwards ? n - 1 - i : i; }

// every thread of every span of k_tsdf_integrate: spans = ceil(nx / 64) * ny * nz, x fastest
static void run_integrate(const pm::TsdfIntegrateArgs& a, bool backwards) {
  const pm::TsdfGrid& g = a.grid;
  const long long x_spans = (g.nx + pm::kTsdfLanes - 1) / pm::kTsdfLanes, spans = x_spans * g.ny * g.nz;
  for (long long b = 0; b < spans; ++b) {
    const long long s = nth(b, spans, backwards), row = s / x_spans;
    int sums[2] = {0, 0};
    for (int l = 0; l < pm::kTsdfLanes; ++l) {
      const int i = (int)((s - row * x_spans) * pm::kTsdfLanes + nth(l, pm::kTsdfLanes, backwards));
      const int k = (int)(row / g.ny), j = (int)(row - (long long)k * g.ny);
      const unsigned flags = i < g.nx ? pm::tsdf_integrate_lane(a, i, j, k) : 0u;
      sums[0] += flags & 1u, sums[1] += (flags >> 1) & 1u;
    }
    for (int c = 0; c < 2; ++c)
      if (sums[c]) pm::reproject_add(a.counts + c, sums[c]);
  }
}

// every thread of every block of k_tsdf_raycast: grid (ceil(cols / 64), ceil(rows / 4)), block (64, 4)
static void run_raycast(const pm::TsdfRaycastArgs& a, bool backwards) {
  const int bx = pm::kTsdfLanes, by = pm::kTsdfWaves;
  const int gx = (a.cols + bx - 1) / bx, gy = (a.rows + by - 1) / by;
  for (int b = 0; b < gx * gy; ++b) {
    const int block = (int)nth(b, gx * gy, backwards);
    int sum = 0;
    for (int i = 0; i < bx * by; ++i) {
      const int t = (int)nth(i, bx * by, backwards);
      const int x = (block % gx) * bx + t % bx, y = (block / gx) * by + t / bx;
      sum += x < a.cols && y < a.rows && pm::tsdf_ray_lane(a, x, y) ? 1 : 0;
    }
    if (sum) pm::reproject_add(a.counts, sum);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = std::string(argv[1]) + "/";
  std::unique_ptr<uint8_t[]> raw;
  if (!read_npy(dir + "params.npy", kParams * sizeof(double), &raw)) return 2;
  double p[kParams];
  memcpy(p, raw.get(), sizeof p);
  pm_tsdf_volume vol = {};
  vol.nx = (int)p[0], vol.ny = (int)p[1], vol.nz = (int)p[2];
  for (int i = 0; i < 3; ++i) vol.origin[i] = p[3 + i];
  vol.voxel = p[6], vol.trunc = p[7], vol.max_weight = (float)p[8];
  const pm_cloud_camera camera = {p[9], p[10], p[11], p[12], p[13]};
  const int rows = (int)p[14], cols = (int)p[15], n = (int)p[16];
  if (vol.nx < 1 || vol.ny < 1 || vol.nz < 1 || rows < 1 || cols < 1 || n < 1 || n > kMaxIntegrates) return 2;
  const size_t vox = (size_t)vol.nx * vol.ny * vol.nz, px = (size_t)rows * cols;
  std::unique_ptr<uint8_t[]> start, disp_b, w_b, want_vox, want_counts, want_disp, want_normals, want_hits;
  if (!read_npy(dir + "start.npy", 8 * vox, &start) || !read_npy(dir + "disp.npy", 4 * px * n, &disp_b) ||
      !read_npy(dir + "weights.npy", 4 * px * n, &w_b) || !read_npy(dir + "want_voxels.npy", 8 * vox * n, &want_vox) ||
      !read_npy(dir + "want_counts.npy", 8 * (size_t)n, &want_counts) || !read_npy(dir + "want_disp.npy", 4 * px, &want_disp) ||
      !read_npy(dir + "want_normals.npy", 12 * px, &want_normals) || !read_npy(dir + "want_hits.npy", 4, &want_hits))
    return 2;
  auto plane = [&](const uint8_t* from) {  // exactly sized allocations
    std::unique_ptr<float[]> q(new float[px]);
    memcpy(q.get(), from, 4 * px);
    return q;
  };
  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const bool backwards = pass == 1;
    const char* const name = backwards ? "backwards" : "forwards";
    std::unique_ptr<pm::TsdfVoxel[]> voxels(new pm::TsdfVoxel[vox]);
    memcpy(voxels.get(), start.get(), 8 * vox);
    for (int k = 0; k < n; ++k) {
      std::unique_ptr<float[]> disp = plane(disp_b.get() + 4 * px * k), weight;
      if (p[19] != 0.0) weight = plane(w_b.get() + 4 * px * k);
      int counts[2] = {0, 0};
      pm::TsdfIntegrateArgs a = {};
      a.cam = pm::cloud_cam(camera);
      a.grid = pm::tsdf_grid(vol);
      const double* m = p + kHead + 12 + 12 * k;
      for (int i = 0; i < 9; ++i) a.R[i] = m[i];
      for (int i = 0; i < 3; ++i) a.t[i] = m[9 + i];
      a.min_disp = (float)p[17], a.max_range = (float)p[18];
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
    const double* m = p + kHead;
    for (int i = 0; i < 9; ++i) r.R[i] = m[i];
    pm::motion_inverse(m, m + 9, r.Ri, r.c);  // as pm_tsdf_raycast forms it on the host
    r.min_range = (double)(float)p[20], r.max_range = (double)(float)p[21];
    r.ds = (double)(float)p[22] * vol.trunc;
    r.min_weight = (float)p[23];
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
