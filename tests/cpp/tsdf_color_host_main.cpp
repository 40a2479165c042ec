// tsdf_color_host_main.cpp -- runs the per-thread code of pm_tsdf_integrate_color, pm_tsdf_color_map and pm_tsdf_color_points
// (csrc/pm_tsdf_color_body.hpp: tsdf_integrate_color_lane, tsdf_color_map_lane and tsdf_color_point_lane, the bodies of the
// kernels of csrc/pm_tsdf_color.hpp) on the HOST, so that tests/test_tsdf_color.py can hold it to the definition
// (tests/tsdf_color_ref.py) without a GPU and under -fsanitize=address,undefined.  Every buffer is a heap allocation of EXACTLY the
// bytes the stage may touch.  One integrate into a distance and a colour volume, then the map gather and the point gather on what
// it left; all of it twice, spans / blocks and threads (host_launch.hpp's walk over the body header's kTsdfBlockX / Y) forwards
// and then backwards: no voxel, pixel or point is touched by two threads, only integer addition crosses them.  Each gather then
// once more with each output alone and with the count alone.  Compiled as HIP source with the host-only switch of hipcc and
// -ffp-contract=off.
//   tsdf_color_host_main <dir>
// <dir> holds .npy dumps (host_npy.hpp: Case): params.npy (float64: nx, ny, nz, origin[3], voxel, trunc, max_weight, fx, fy, cx,
// cy, baseline, rows, cols, min_disp, max_range, band, has_weight, float_image, min_weight, byte_scale, n (points), d_n (2^31: not
// given), the integrate's pose (R[9], t[3]), the map gather's pose), start_voxels.npy (float32 [nz][ny][nx][2]), start_colors.npy
// (float32 [nz][ny][nx][4]), disp.npy, weights.npy (float32 [rows][cols]; read only where has_weight), image.npy (uint8 or float32
// [rows][cols][3]), map_disp.npy (float32 [rows][cols]: the map whose pixels are coloured), xyz.npy (float32 [n][3]),
// start_bgr.npy / start_bgr8.npy (float32 / uint8 [n][3]: the point outputs before the call) and the definition's results
// want_voxels.npy, want_colors.npy, want_counts.npy (int32 [3]), want_map_bgr.npy, want_map_bgr8.npy, want_map_count.npy (int32
// [1]), want_pts_bgr.npy, want_pts_bgr8.npy, want_pts_count.npy.
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.

#include "host_launch.hpp"
#include "host_npy.hpp"
#include "pm_tsdf_color_body.hpp"

enum { kNx, kNy, kNz, kOrigin, kVoxel = kOrigin + 3, kTrunc, kMaxWeight, kFx, kFy, kCx, kCy, kBaseline, kRows, kCols, kMinDisp,
       kMaxRange, kBand, kHasWeight, kFloatImage, kMinWeight, kByteScale, kN, kDn, kPose, kMapPose = kPose + 12,
       kParams = kMapPose + 12 };

// every thread of every span of k_tsdf_integrate_color: a wavefront per span, the spans ceil(nx / 64) x ny x nz, x fastest
static void run_integrate(const pm::TsdfIntegrateColorArgs& a, bool backwards) {
  const pm::TsdfGrid& g = a.base.grid;
  for_blocks((g.nx + pm::kTsdfLanes - 1) / pm::kTsdfLanes, g.ny, g.nz, backwards, [&](int span, int j, int k) {
    int sums[3] = {0, 0, 0};  // in view, updated, coloured
    for_threads(pm::kTsdfBlockX, 1, backwards, [&](int lane, int) {
      const int i = span * pm::kTsdfLanes + lane;
      add_flags<1>(i < g.nx ? pm::tsdf_integrate_color_lane(a, i, j, k) : 0u, sums);
    });
    flush_sums(a.base.counts, sums, pm::reproject_add);
  });
}

// every thread of every block of k_tsdf_color_map: grid (ceil(cols / 64), ceil(rows / 4))
static void run_map(const pm::TsdfColorMapArgs& a, bool backwards) {
  const int gx = (a.cols + pm::kTsdfBlockX - 1) / pm::kTsdfBlockX, gy = (a.rows + pm::kTsdfBlockY - 1) / pm::kTsdfBlockY;
  for_blocks(gx, gy, 1, backwards, [&](int bx, int by, int) {
    int sums[1] = {0};
    for_threads(pm::kTsdfBlockX, pm::kTsdfBlockY, backwards, [&](int tx, int ty) {
      const int x = bx * pm::kTsdfBlockX + tx, y = by * pm::kTsdfBlockY + ty;
      sums[0] += x < a.cols && y < a.rows && pm::tsdf_color_map_lane(a, x, y) ? 1 : 0;
    });
    flush_sums(a.s.counts, sums, pm::reproject_add);
  });
}

// every thread of every block of k_tsdf_color_points: grid (ceil(n / 256))
static void run_points(const pm::TsdfColorPointsArgs& a, bool backwards) {
  const int per_block = pm::kTsdfBlockX * pm::kTsdfBlockY;
  for_blocks((a.n + per_block - 1) / per_block, 1, 1, backwards, [&](int b, int, int) {
    int sums[1] = {0};
    for_threads(pm::kTsdfBlockX, pm::kTsdfBlockY, backwards, [&](int tx, int ty) {
      const long long at = ((long long)b * pm::kTsdfBlockY + ty) * pm::kTsdfLanes + tx;
      sums[0] += at < (long long)pm::tsdf_color_points_limit(a) && pm::tsdf_color_point_lane(a, (int)at) ? 1 : 0;
    });
    flush_sums(a.s.counts, sums, pm::reproject_add);
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
  const bool float_image = p[kFloatImage] != 0.0;
  if (c.failed || vol.nx < 1 || vol.ny < 1 || vol.nz < 1 || rows < 1 || cols < 1 || n < 0) return 2;
  const size_t vox = (size_t)vol.nx * vol.ny * vol.nz, px = (size_t)rows * cols, image_bytes = (float_image ? 12 : 3) * px;
  const auto start_vox = c.raw("start_voxels", 8 * vox), start_col = c.raw("start_colors", 16 * vox);
  const auto disp_b = c.raw("disp", 4 * px), w_b = c.raw("weights", 4 * px), image_b = c.raw("image", image_bytes);
  const auto map_disp_b = c.raw("map_disp", 4 * px), xyz_b = c.raw("xyz", 12 * (size_t)n);
  const auto start_bgr = c.raw("start_bgr", 12 * (size_t)n), start_bgr8 = c.raw("start_bgr8", 3 * (size_t)n);
  const auto want_vox = c.raw("want_voxels", 8 * vox), want_col = c.raw("want_colors", 16 * vox), want_counts = c.raw("want_counts", 12);
  const auto want_map_bgr = c.raw("want_map_bgr", 12 * px), want_map_bgr8 = c.raw("want_map_bgr8", 3 * px);
  const auto want_map_count = c.raw("want_map_count", 4);
  const auto want_pts_bgr = c.raw("want_pts_bgr", 12 * (size_t)n), want_pts_bgr8 = c.raw("want_pts_bgr8", 3 * (size_t)n);
  const auto want_pts_count = c.raw("want_pts_count", 4);
  if (c.failed) return 2;
  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const bool backwards = pass == 1;
    const char* const name = backwards ? "backwards" : "forwards";
    const auto voxels = exact_copy<pm::TsdfVoxel>(start_vox.get(), vox);
    // (operator new aligns to 16 bytes: the colour records' alignment)
    const auto colors = exact_copy<pm::TsdfColor>(start_col.get(), vox);
    {
      std::unique_ptr<float[]> disp = exact_copy<float>(disp_b.get(), px), weight;
      if (p[kHasWeight] != 0.0) weight = exact_copy<float>(w_b.get(), px);
      const auto image = exact_copy<uint8_t>(image_b.get(), image_bytes);
      int counts[3] = {0, 0, 0};
      pm::TsdfIntegrateColorArgs a = {};
      a.base.cam = pm::cloud_cam(camera);
      a.base.grid = pm::tsdf_grid(vol);
      read_motion(&p[kPose], a.base.R, a.base.t);
      a.base.min_disp = (float)p[kMinDisp], a.base.max_range = (float)p[kMaxRange];
      a.base.disp = disp.get(), a.base.weight = weight.get(), a.base.rows = rows, a.base.cols = cols;
      a.base.voxels = voxels.get(), a.base.counts = counts;
      a.bandw = (double)(float)p[kBand] * vol.trunc;  // as pm_tsdf_integrate_color forms it on the host
      a.bgr8 = float_image ? nullptr : image.get();
      a.bgr = float_image ? reinterpret_cast<const float*>(image.get()) : nullptr;
      a.colors = colors.get();
      run_integrate(a, backwards);
      bad |= differ("the distance volume", voxels.get(), want_vox.get(), 8 * vox, name);
      bad |= differ("the colour volume", colors.get(), want_col.get(), 16 * vox, name);
      bad |= differ("the integrate's counts", counts, want_counts.get(), 12, name);
      bad |= differ("the input map", disp.get(), disp_b.get(), 4 * px, name);  // read only
      bad |= differ("the input image", image.get(), image_b.get(), image_bytes, name);
    }
    pm::TsdfColorSampler s = {};
    s.grid = pm::tsdf_grid(vol);
    s.min_weight = (float)p[kMinWeight], s.byte_scale = (float)p[kByteScale];
    s.colors = colors.get();
    for (int outs = 3; outs >= 0; --outs) {  // both outputs, the bytes alone, the floats alone, the count alone
      static const char* const which[4] = {"count alone", "floats alone", "bytes alone", "both outputs"};
      const std::string label = std::string(name) + ", " + which[outs];
      {
        const auto map_disp = exact_copy<float>(map_disp_b.get(), px);
        std::unique_ptr<float[]> bgr;
        std::unique_ptr<uint8_t[]> bgr8;
        if (outs & 1) bgr.reset(new float[3 * px]);
        if (outs & 2) bgr8.reset(new uint8_t[3 * px]);
        int count = 0;
        pm::TsdfColorMapArgs m = {};
        m.s = s;
        m.s.bgr_out = bgr.get(), m.s.bgr8_out = bgr8.get(), m.s.counts = &count;
        m.cam = pm::cloud_cam(camera);
        double R[9], t[3];
        read_motion(&p[kMapPose], R, t);
        pm::motion_inverse(R, t, m.Ri, m.c);  // as pm_tsdf_color_map forms it on the host
        m.disp = map_disp.get(), m.rows = rows, m.cols = cols;
        run_map(m, backwards);
        if (outs & 1) bad |= differ("the map's floats", bgr.get(), want_map_bgr.get(), 12 * px, label.c_str());
        if (outs & 2) bad |= differ("the map's bytes", bgr8.get(), want_map_bgr8.get(), 3 * px, label.c_str());
        bad |= differ("the map's count", &count, want_map_count.get(), 4, label.c_str());
      }
      {
        const size_t m3 = 3 * (size_t)n;
        const auto xyz = exact_copy<float>(xyz_b.get(), m3);
        std::unique_ptr<float[]> bgr;
        std::unique_ptr<uint8_t[]> bgr8;
        if (outs & 1) bgr = exact_copy<float>(start_bgr.get(), m3);
        if (outs & 2) bgr8 = exact_copy<uint8_t>(start_bgr8.get(), m3);
        int count = 0;
        const std::unique_ptr<int> d_n(p[kDn] < 2147483648.0 ? new int((int)p[kDn]) : nullptr);  // 2^31: not given
        pm::TsdfColorPointsArgs q = {};
        q.s = s;
        q.s.bgr_out = bgr.get(), q.s.bgr8_out = bgr8.get(), q.s.counts = &count;
        q.xyz = xyz.get(), q.n = n, q.d_n = d_n.get();
        run_points(q, backwards);
        if (outs & 1) bad |= differ("the points' floats", bgr.get(), want_pts_bgr.get(), 4 * m3, label.c_str());
        if (outs & 2) bad |= differ("the points' bytes", bgr8.get(), want_pts_bgr8.get(), m3, label.c_str());
        bad |= differ("the points' count", &count, want_pts_count.get(), 4, label.c_str());
      }
    }
    bad |= differ("the colour volume behind the gathers", colors.get(), want_col.get(), 16 * vox, name);  // read only
  }
  return bad ? 1 : 0;
}
