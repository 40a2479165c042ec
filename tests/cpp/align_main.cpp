// Drives AlignDisparity, ComposeMotion and TsdfVolume::Align of the C++ mirror (ocean-perception_amd/host/imaging.hpp) like a host
// caller, and pm_align_disparity of the C ABI beside them.  Reads raw inputs written by tests/test_cpp_align.py and writes raw
// outputs for it to compare with the definition (tests/align_ref.py, tests/tsdf_ref.py).
//   align_main <dir> <rows> <cols>   in: camera.f64 (fx, fy, cx, cy, baseline), options.f64 (min_disp, max_diff, huber_px,
//                                    iterations, epsilon, min_used), guess.f64 (R[9], t[3]), disp_model.f32, normals_model.f32
//                                    ([rows][cols][3]), disp_new.f32, grid.f64 (nx, ny, nz, origin[3], voxel, trunc, max_weight),
//                                    ray.f32 (min_range, max_range, step, min_weight), pose.f64 (R[9], t[3]: where the volume saw
//                                    disp_model from and where Align starts);  out: motion.f64 and info.f64 (AlignDisparity:
//                                    R[9], t[3]; valid, n_model, n_gate, n_used, iterations, rms_px, H[21]), abi_motion.f64 and
//                                    abi_info.f64 (pm_align_disparity on buffers of the program's own), composed.f64
//                                    (ComposeMotion(motion, pose)), tracked.f64 and tracked_info.f64 (TsdfVolume::Align)
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

static std::vector<double> flat(const pm_align_info& i) {
  std::vector<double> v = {(double)i.valid, (double)i.n_model, (double)i.n_gate, (double)i.n_used, (double)i.iterations, i.rms_px};
  v.insert(v.end(), i.H, i.H + 21);
  return v;
}

static Motion motion_of(const double* p) {
  Motion m;
  for (size_t i = 0; i < 9; ++i) m.R[i] = p[i];
  for (size_t i = 0; i < 3; ++i) m.t[i] = p[9 + i];
  return m;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::string dir = argv[1];
  const int rows = atoi(argv[2]), cols = atoi(argv[3]);
  if (rows < 1 || cols < 1) return 2;
  try {
    const size_t px = (size_t)rows * cols;
    double c[5], o[6], gv[12], g[9], pv[12];
    float r[4];
    bm::core::Image<float> disp_model(rows, cols), disp_new(rows, cols);
    bm::core::Image<bm::core::Vec3f> normals(rows, cols);
    if (!read_raw(dir + "/camera.f64", c, 5) || !read_raw(dir + "/options.f64", o, 6) || !read_raw(dir + "/guess.f64", gv, 12) ||
        !read_raw(dir + "/disp_model.f32", disp_model) || !read_raw(dir + "/disp_new.f32", disp_new) ||
        !read_raw(dir + "/normals_model.f32", reinterpret_cast<float*>(normals.data()), 3 * px) ||
        !read_raw(dir + "/grid.f64", g, 9) || !read_raw(dir + "/ray.f32", r, 4) || !read_raw(dir + "/pose.f64", pv, 12)) {
      std::cerr << "cannot read inputs\n";
      return 3;
    }
    StereoModel model;
    model.fx = c[0], model.fy = c[1], model.cx = c[2], model.cy = c[3], model.baseline = c[4];
    AlignOptions opt;
    opt.min_disp = (float)o[0], opt.max_diff = (float)o[1], opt.huber_px = o[2], opt.iterations = (int)o[3], opt.epsilon = o[4];
    opt.min_used = (int)o[5];
    const Motion guess = motion_of(gv), pose = motion_of(pv);
    bm::pm::PatchmatchGpu unplanned{bm::pm::PatchmatchGpu::Params()};
    try {
      AlignDisparity(unplanned, model, opt, &guess, disp_model, normals, disp_new);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    bm::pm::PatchmatchGpu::Params params;
    params.max_rows = rows, params.max_cols = cols;
    bm::pm::PatchmatchGpu matcher(params);
    pm_align_info info;
    const Motion m = AlignDisparity(matcher, model, opt, &guess, disp_model, normals, disp_new, &info);
    write_raw(dir + "/motion.f64", flat(m).data(), 12);
    write_raw(dir + "/info.f64", flat(info).data(), 27);
    {  // the C ABI on buffers of the program's own
      pm_handle* h = matcher.handle();
      void *d_model = nullptr, *d_normals = nullptr, *d_new = nullptr;
      if (pm_device_malloc(h, 4 * px, &d_model) || pm_device_malloc(h, 12 * px, &d_normals) || pm_device_malloc(h, 4 * px, &d_new)) return 4;
      pm_upload(h, d_model, disp_model.data(), 4 * px);
      pm_upload(h, d_normals, normals.data(), 12 * px);
      pm_upload(h, d_new, disp_new.data(), 4 * px);
      const pm_cloud_camera cam = {c[0], c[1], c[2], c[3], c[4]};
      const pm_align_options copt = {opt.min_disp, opt.max_diff, opt.huber_px, opt.iterations, opt.epsilon, opt.min_used};
      pm_motion cg, out;
      for (int i = 0; i < 9; ++i) cg.R[i] = gv[i];
      for (int i = 0; i < 3; ++i) cg.t[i] = gv[9 + i];
      pm_align_info ci;
      const int rc = pm_align_disparity(h, &cam, &copt, &cg, (const float*)d_model, (const float*)d_normals, (const float*)d_new, rows,
                                        cols, &out, &ci);
      pm_device_free(h, d_model), pm_device_free(h, d_normals), pm_device_free(h, d_new);
      if (rc != PM_OK) return 5;
      Motion am;
      for (size_t i = 0; i < 9; ++i) am.R[i] = out.R[i];
      for (size_t i = 0; i < 3; ++i) am.t[i] = out.t[i];
      write_raw(dir + "/abi_motion.f64", flat(am).data(), 12);
      write_raw(dir + "/abi_info.f64", flat(ci).data(), 27);
    }
    write_raw(dir + "/composed.f64", flat(ComposeMotion(m, pose)).data(), 12);
    bm::core::Image<float> other(rows + 1, cols);
    try {
      AlignDisparity(matcher, model, opt, &guess, disp_model, normals, other);
      return 6;
    } catch (const std::invalid_argument& e) {
      std::printf("refused: %s\n", e.what());
    }
    AlignOptions bad = opt;
    bad.min_used = 3;
    try {
      AlignDisparity(matcher, model, bad, &guess, disp_model, normals, disp_new);
      return 6;
    } catch (const std::runtime_error& e) {
      std::printf("refused: %s\n", e.what());
    }
    // tracking against the model: the volume sees disp_model from `pose`, the new frame is aligned against its render there
    TsdfGrid grid;
    grid.nx = (int)g[0], grid.ny = (int)g[1], grid.nz = (int)g[2];
    grid.origin = {{g[3], g[4], g[5]}};
    grid.voxel = g[6], grid.trunc = g[7], grid.max_weight = (float)g[8];
    TsdfRaycastOptions ray;
    ray.min_range = r[0], ray.max_range = r[1], ray.step = r[2], ray.min_weight = r[3];
    TsdfVolume volume(matcher, grid);
    volume.Integrate(model, pose, disp_model);
    pm_align_info ti;
    const Motion tracked = volume.Align(model, pose, disp_new, ray, opt, &ti);
    write_raw(dir + "/tracked.f64", flat(tracked).data(), 12);
    write_raw(dir + "/tracked_info.f64", flat(ti).data(), 27);
    const Motion again = volume.Align(model, pose, disp_new, ray, opt);  // the buffers of the first call serve the second
    if (flat(again) != flat(tracked)) return 7;
    std::printf("ok valid=%d used=%d iterations=%d tracked_valid=%d\n", info.valid, info.n_used, info.iterations, ti.valid);
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << "\n";
    return 10;
  }
}
