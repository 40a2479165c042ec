// Drives AlignColorDisparity and TsdfVolume::AlignColor of the C++ mirror (ocean-perception_amd/host/imaging.hpp) like a host
// caller, and pm_align_color_disparity and pm_align_sums_blend of the C ABI beside them.  Reads raw inputs written by
// tests/test_cpp_align_color.py and writes raw outputs for it to compare with the definition (tests/align_photo_ref.py).
//   align_color_main <dir> <rows> <cols>
//     in:  camera.f64 (fx, fy, cx, cy, baseline), options.f64 (min_disp, max_diff, huber_px, iterations, epsilon, min_used,
//          huber_levels, lambda), guess.f64 (R[9], t[3]), disp_model.f32, normals_model.f32 and bgr_model.f32 ([rows][cols][3]),
//          disp_new.f32, bgr_new.f32 ([rows][cols][3]), bgr8_new.u8 ([rows][cols][3]), grid.f64 (nx, ny, nz, origin[3], voxel,
//          trunc, max_weight), ray.f32 (min_range, max_range, step, min_weight), band.f32, pose.f64 (R[9], t[3]: where the volume saw
//          disp_model and bgr_model from and where AlignColor starts), sums.f64 (two records' 28 doubles and 3 counts each, then lambda)
//     out: motion.f64, info.f64 (AlignColorDisparity with the float image: R[9], t[3]; the info flattened as `flat` below),
//          motion8.f64, info8.f64 (with the byte image), abi_motion.f64, abi_info.f64 (pm_align_color_disparity, bytes, on buffers
//          of the program's own), tracked.f64, tracked_info.f64 (TsdfVolume::AlignColor, bytes), blend.f64 (pm_align_sums_blend:
//          28 doubles and 3 counts, out aliasing the geometric record)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "imaging.hpp"
#include "raw_io.hpp"

using namespace bm::imaging;

static std::vector<double> flat(const Motion& m) {
  std::vector<double> v(m.R.begin(), m.R.end());
  v.insert(v.end(), m.t.begin(), m.t.end());
  return v;
}

static std::vector<double> flat(const pm_align_color_info& i) {
  std::vector<double> v = {(double)i.geo.valid, (double)i.geo.n_model, (double)i.geo.n_gate, (double)i.geo.n_used,
                           (double)i.geo.iterations, i.geo.rms_px};
  v.insert(v.end(), i.geo.H, i.geo.H + 21);
  v.insert(v.end(), {(double)i.n_photo_model, (double)i.n_photo_gate, (double)i.n_photo_used, i.rms_levels});
  v.insert(v.end(), i.H, i.H + 21);
  return v;  // 52
}

static Motion motion_of(const double* p) {
  Motion m;
  for (size_t i = 0; i < 9; ++i) m.R[i] = p[i];
  for (size_t i = 0; i < 3; ++i) m.t[i] = p[9 + i];
  return m;
}

static pm_align_sums sums_of(const double* p) {
  pm_align_sums s = {};
  for (int i = 0; i < 28; ++i) reinterpret_cast<double*>(&s)[i] = p[i];
  s.n_model = (int)p[28], s.n_gate = (int)p[29], s.n_used = (int)p[30];
  return s;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::string dir = argv[1];
  const int rows = atoi(argv[2]), cols = atoi(argv[3]);
  if (rows < 1 || cols < 1) return 2;
  try {
    const size_t px = (size_t)rows * cols;
    double c[5], o[8], gv[12], g[9], pv[12], sv[63];
    float r[4], band;
    bm::core::Image<float> disp_model(rows, cols), disp_new(rows, cols);
    bm::core::Image<bm::core::Vec3f> normals(rows, cols), bgr_model(rows, cols), bgr_new(rows, cols);
    bm::core::Image<bm::core::Vec3b> bgr8_new(rows, cols);
    if (!read_raw(dir + "/camera.f64", c, 5) || !read_raw(dir + "/options.f64", o, 8) || !read_raw(dir + "/guess.f64", gv, 12) ||
        !read_raw(dir + "/disp_model.f32", disp_model) || !read_raw(dir + "/disp_new.f32", disp_new) ||
        !read_raw(dir + "/normals_model.f32", reinterpret_cast<float*>(normals.data()), 3 * px) ||
        !read_raw(dir + "/bgr_model.f32", reinterpret_cast<float*>(bgr_model.data()), 3 * px) ||
        !read_raw(dir + "/bgr_new.f32", reinterpret_cast<float*>(bgr_new.data()), 3 * px) ||
        !read_raw(dir + "/bgr8_new.u8", reinterpret_cast<uint8_t*>(bgr8_new.data()), 3 * px) ||
        !read_raw(dir + "/grid.f64", g, 9) || !read_raw(dir + "/ray.f32", r, 4) || !read_raw(dir + "/band.f32", &band, 1) ||
        !read_raw(dir + "/pose.f64", pv, 12) || !read_raw(dir + "/sums.f64", sv, 63)) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    {  // host only: the blend, out aliasing geo
      pm_align_sums geo = sums_of(sv), photo = sums_of(sv + 31);
      if (pm_align_sums_blend(&geo, nullptr, sv[62], &geo) != PM_ERR_INVALID_ARG) return 8;
      if (pm_align_sums_blend(&geo, &photo, sv[62], &geo) != PM_OK) return 8;
      std::vector<double> v(reinterpret_cast<double*>(&geo), reinterpret_cast<double*>(&geo) + 28);
      v.insert(v.end(), {(double)geo.n_model, (double)geo.n_gate, (double)geo.n_used});
      write_raw(dir + "/blend.f64", v.data(), 31);
    }
    StereoModel model;
    model.fx = c[0], model.fy = c[1], model.cx = c[2], model.cy = c[3], model.baseline = c[4];
    AlignColorOptions opt;
    opt.align.min_disp = (float)o[0], opt.align.max_diff = (float)o[1], opt.align.huber_px = o[2], opt.align.iterations = (int)o[3];
    opt.align.epsilon = o[4], opt.align.min_used = (int)o[5], opt.huber_levels = o[6], opt.lambda = o[7];
    const Motion guess = motion_of(gv), pose = motion_of(pv);
    bm::pm::PatchmatchGpu::Params params;
    params.max_rows = rows, params.max_cols = cols;
    bm::pm::PatchmatchGpu matcher(params);
    pm_align_color_info info, info8;
    const Motion m = AlignColorDisparity(matcher, model, opt, &guess, disp_model, normals, bgr_model, disp_new, bgr_new, &info);
    write_raw(dir + "/motion.f64", flat(m).data(), 12);
    write_raw(dir + "/info.f64", flat(info).data(), 52);
    const Motion m8 = AlignColorDisparity(matcher, model, opt, &guess, disp_model, normals, bgr_model, disp_new, bgr8_new, &info8);
    write_raw(dir + "/motion8.f64", flat(m8).data(), 12);
    write_raw(dir + "/info8.f64", flat(info8).data(), 52);
    {  // the C ABI on buffers of the program's own
      pm_handle* h = matcher.handle();
      void *d_model = nullptr, *d_normals = nullptr, *d_bgr = nullptr, *d_new = nullptr, *d_bgr8 = nullptr;
      if (pm_device_malloc(h, 4 * px, &d_model) || pm_device_malloc(h, 12 * px, &d_normals) || pm_device_malloc(h, 12 * px, &d_bgr) ||
          pm_device_malloc(h, 4 * px, &d_new) || pm_device_malloc(h, 3 * px, &d_bgr8))
        return 4;
      pm_upload(h, d_model, disp_model.data(), 4 * px);
      pm_upload(h, d_normals, normals.data(), 12 * px);
      pm_upload(h, d_bgr, bgr_model.data(), 12 * px);
      pm_upload(h, d_new, disp_new.data(), 4 * px);
      pm_upload(h, d_bgr8, bgr8_new.data(), 3 * px);
      const pm_cloud_camera cam = {c[0], c[1], c[2], c[3], c[4]};
      const pm_align_color_options copt = {{opt.align.min_disp, opt.align.max_diff, opt.align.huber_px, opt.align.iterations,
                                            opt.align.epsilon, opt.align.min_used},
                                           opt.huber_levels, opt.lambda};
      pm_motion cg, out;
      for (int i = 0; i < 9; ++i) cg.R[i] = gv[i];
      for (int i = 0; i < 3; ++i) cg.t[i] = gv[9 + i];
      pm_align_color_info ci;
      const int rc = pm_align_color_disparity(h, &cam, &copt, &cg, (const float*)d_model, (const float*)d_normals, (const float*)d_bgr,
                                              (const float*)d_new, (const uint8_t*)d_bgr8, nullptr, rows, cols, &out, &ci);
      pm_device_free(h, d_model), pm_device_free(h, d_normals), pm_device_free(h, d_bgr), pm_device_free(h, d_new);
      pm_device_free(h, d_bgr8);
      if (rc != PM_OK) return 5;
      std::vector<double> am(out.R, out.R + 9);
      am.insert(am.end(), out.t, out.t + 3);
      write_raw(dir + "/abi_motion.f64", am.data(), 12);
      write_raw(dir + "/abi_info.f64", flat(ci).data(), 52);
    }
    bm::core::Image<bm::core::Vec3b> other(rows + 1, cols);
    try {
      AlignColorDisparity(matcher, model, opt, &guess, disp_model, normals, bgr_model, disp_new, other);
      return 6;
    } catch (const std::invalid_argument& e) {
      std::printf("refused: %s\n", e.what());
    }
    AlignColorOptions bad = opt;
    bad.lambda = -1.0;
    try {
      AlignColorDisparity(matcher, model, bad, &guess, disp_model, normals, bgr_model, disp_new, bgr8_new);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    // tracking against the coloured model: the volume sees disp_model and bgr_model from `pose`
    TsdfGrid grid;
    grid.nx = (int)g[0], grid.ny = (int)g[1], grid.nz = (int)g[2];
    grid.origin = {{g[3], g[4], g[5]}};
    grid.voxel = g[6], grid.trunc = g[7], grid.max_weight = (float)g[8];
    TsdfRaycastOptions ray;
    ray.min_range = r[0], ray.max_range = r[1], ray.step = r[2], ray.min_weight = r[3];
    {
      TsdfVolume grey(matcher, grid);
      try {
        grey.AlignColor(model, pose, disp_new, bgr8_new, ray, opt);
        return 6;
      } catch (const std::logic_error& e) {
        std::printf("refused: %s\n", e.what());
      }
    }
    TsdfVolume volume(matcher, grid, /*with_color=*/true);
    TsdfColorOptions co;
    co.band = band;
    volume.IntegrateColor(model, pose, disp_model, bgr_model, nullptr, co);
    pm_align_color_info ti;
    const Motion tracked = volume.AlignColor(model, pose, disp_new, bgr8_new, ray, opt, TsdfColorSampleOptions(), &ti);
    write_raw(dir + "/tracked.f64", flat(tracked).data(), 12);
    write_raw(dir + "/tracked_info.f64", flat(ti).data(), 52);
    std::printf("ok valid=%d photo_used=%d iterations=%d tracked_valid=%d\n", info.geo.valid, info.n_photo_used, info.geo.iterations,
                ti.geo.valid);
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
