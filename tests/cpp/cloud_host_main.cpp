// cloud_host_main.cpp -- runs the point-cloud stages' own per-thread code (csrc/pm_cloud_body.hpp: backproject_four,
// cloud_item, cloud_store, cloud_normal -- the bodies of the kernels of csrc/pm_cloud.hpp and of k_planes_normals) on the
// HOST, so that tests/test_pointcloud.py can hold it to the definition (tests/pointcloud_ref.py) without a GPU and under
// -fsanitize=address,undefined.  Every buffer is a heap allocation of EXACTLY the bytes the stage may touch: a load past the
// last disparity, or a store behind slot min(count, capacity) - 1, is reported.  Compiled as HIP source with the host-only
// switch of hipcc and -ffp-contract=off.
//   cloud_host_main <dir>
// <dir> holds .npy dumps (host_npy.hpp: Case): params.npy (float64: rows, cols, fx, fy, cx, cy, baseline, min_disp, max_range,
// stride, capacity, shift), disp.npy (float32 [rows][cols]), planes.npy (float32 [3][rows][cols]: a, b, z), bgr.npy (uint8
// [rows][cols][3]) and the definition's results want_xyz.npy, want_normals.npy (masked by disp), want_count.npy (int32 [1]),
// want_cloud_xyz.npy, want_cloud_normals.npy, want_cloud_bgr.npy, want_cloud_index.npy (each with min(count, capacity)
// entries).  shift: the organised outputs start `shift` floats into their allocation (an unaligned destination for shift % 4 != 0).
// Exit status 0: every result equals its dump byte for byte; 1: a mismatch (named on stderr); 2: bad input.

#include "host_npy.hpp"
#include "pm_cloud_body.hpp"

enum { kRows, kCols, kFx, kFy, kCx, kCy, kBaseline, kMinDisp, kMaxRange, kStride, kCapacity, kShift, kParams };

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Case c(argv[1]);
  const std::vector<double> p = c.params(kParams);
  const int rows = (int)p[kRows], cols = (int)p[kCols], stride = (int)p[kStride], capacity = (int)p[kCapacity], shift = (int)p[kShift];
  const pm_cloud_camera camera = {p[kFx], p[kFy], p[kCx], p[kCy], p[kBaseline]};
  const pm_cloud_filter filter = {(float)p[kMinDisp], (float)p[kMaxRange], stride};
  if (c.failed || rows < 1 || cols < 1 || stride < 1 || capacity < 0 || shift < 0) return 2;
  const size_t px = (size_t)rows * cols;
  const auto disp_p = c.read<float>("disp", px), planes_p = c.read<float>("planes", 3 * px);  // aligned like a device allocation
  const auto bgr_b = c.raw("bgr", 3 * px);
  const auto want_xyz = c.raw("want_xyz", 12 * px), want_normals = c.raw("want_normals", 12 * px);
  const auto want_count = c.read<int32_t>("want_count", 1);
  if (c.failed) return 2;
  const float *disp = disp_p.get(), *planes = planes_p.get();
  const pm::CloudCam cam = pm::cloud_cam(camera);
  int bad = 0;

  // pm_backproject: every thread of k_backproject, into an allocation with `shift` floats in front and none behind
  std::unique_ptr<float[]> xyz(new float[shift + 3 * px]);
  for (int k = 0; k < shift; ++k) xyz[k] = -77.f;
  const pm::BackprojectArgs ba = {cam, disp, rows, cols, xyz.get() + shift};
  for (int y = 0; y < rows; ++y)
    for (int x4 = 0; x4 < cols; x4 += 4) pm::backproject_four(ba, x4, y);
  bad |= differ("xyz", xyz.get() + shift, want_xyz.get(), 12 * px);
  for (int k = 0; k < shift; ++k) bad |= xyz[k] != -77.f;

  // pm_planes_normals: cloud_normal per pixel, masked by the map
  std::unique_ptr<float[]> normals(new float[3 * px]);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) {
      const size_t i = (size_t)y * cols + x;
      pm::cloud_normal(cam, planes[i], planes[px + i], planes[2 * px + i], x, y, !(disp[i] > 0.f), normals.get() + 3 * i);
    }
  bad |= differ("normals", normals.get(), want_normals.get(), 12 * px);

  // pm_point_cloud: the items in order, the slot counted as the three launches compute it
  const int want_n = want_count[0];
  if (want_n < 0) return 2;
  const size_t m = (size_t)(want_n < capacity ? want_n : capacity);
  const auto want_cxyz = c.raw("want_cloud_xyz", 12 * m), want_cn = c.raw("want_cloud_normals", 12 * m);
  const auto want_cbgr = c.raw("want_cloud_bgr", 3 * m), want_cidx = c.raw("want_cloud_index", 4 * m);
  if (c.failed) return 2;
  std::unique_ptr<float[]> cxyz(new float[3 * m ? 3 * m : 1]), cn(new float[3 * m ? 3 * m : 1]);
  std::unique_ptr<uint8_t[]> cbgr(new uint8_t[3 * m ? 3 * m : 1]);
  std::unique_ptr<int32_t[]> cidx(new int32_t[m ? m : 1]);
  const pm::CloudArgs ca = pm::cloud_args(camera, filter, disp, rows, cols);
  const pm::CloudStreams cs = {normals.get(), bgr_b.get(), cxyz.get(), cn.get(), cbgr.get(), cidx.get(), capacity};
  long long slot = 0;
  for (long long item = 0; item < ca.items; ++item) {
    int x, y;
    float pt[3];
    if (!pm::cloud_item(ca, item, &x, &y, pt)) continue;
    if (slot < capacity) pm::cloud_store(ca, cs, slot, x, y, pt);
    ++slot;
  }
  if (slot != want_n) {
    fprintf(stderr, "count %lld, the definition counts %d\n", slot, want_n);
    bad = 1;
  }
  bad |= differ("cloud xyz", cxyz.get(), want_cxyz.get(), 12 * m);
  bad |= differ("cloud normals", cn.get(), want_cn.get(), 12 * m);
  bad |= differ("cloud bgr", cbgr.get(), want_cbgr.get(), 3 * m);
  bad |= differ("cloud index", cidx.get(), want_cidx.get(), 4 * m);
  return bad ? 1 : 0;
}
