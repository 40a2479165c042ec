// motion.cpp -- pm_solve_motion (include/pm/imaging.h): the 6-parameter fit of the left camera's motion to the tracks of
// pm_track_features, on the host in binary64.  It is held to tests/motion_ref.py::solve BIT FOR BIT: every operation below is
// one rounding, parentheses and the order of every sum as that file writes them, no trigonometric function and no library
// solver; this unit is compiled with -ffp-contract=off.  It sees the C ABI only, no handle and no HIP header.
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "motion_solve.hpp"
#include "pm/imaging.h"

namespace {

struct Point {
  double X, Y, Z, x_new, y_new;
};

struct Residual {
  bool used;
  double Qx, Qy, Qz, iz, a, b, ru, rv, e2, e;
};

inline Residual residual(const pm_cloud_camera& c, const double R[9], const double t[3], const Point& p) {
  Residual r;
  r.Qx = (((R[0] * p.X) + (R[1] * p.Y)) + (R[2] * p.Z)) + t[0];
  r.Qy = (((R[3] * p.X) + (R[4] * p.Y)) + (R[5] * p.Z)) + t[1];
  r.Qz = (((R[6] * p.X) + (R[7] * p.Y)) + (R[8] * p.Z)) + t[2];
  r.used = r.Qz > 0.0;
  r.iz = 1.0 / r.Qz;
  r.a = r.Qx * r.iz;
  r.b = r.Qy * r.iz;
  r.ru = ((c.fx * r.a) + c.cx) - p.x_new;
  r.rv = ((c.fy * r.b) + c.cy) - p.y_new;
  r.e2 = (r.ru * r.ru) + (r.rv * r.rv);
  r.e = std::sqrt(r.e2);
  return r;
}

}  // namespace

extern "C" int pm_solve_motion(const pm_cloud_camera* camera, const pm_solve_options* options, const pm_track* tracks, int n,
                               const pm_motion* guess, pm_motion* out, pm_motion_info* info) {
  if (!camera || !options || n < 0 || (n > 0 && !tracks) || (!out && !info)) return PM_ERR_INVALID_ARG;
  const double cam[5] = {camera->fx, camera->fy, camera->cx, camera->cy, camera->baseline};
  for (double v : cam)
    if (!std::isfinite(v)) return PM_ERR_INVALID_ARG;
  if (camera->fx == 0.0 || camera->fy == 0.0) return PM_ERR_INVALID_ARG;
  if (options->iterations < 1 || options->iterations > 50 || !(options->huber_px > 0.0) || !(options->epsilon >= 0.0) ||
      !(options->inlier_px > 0.0) || options->min_inliers < 6)
    return PM_ERR_INVALID_ARG;
  pm_motion start = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
  if (guess) {
    start = *guess;
    for (int i = 0; i < 12; ++i)
      if (!std::isfinite(i < 9 ? start.R[i] : start.t[i - 9])) return PM_ERR_INVALID_ARG;
  }
  const pm_cloud_camera& c = *camera;
  const double fxb = c.fx * c.baseline;
  std::vector<Point> pts;
  try {
    pts.reserve((size_t)n);
  } catch (const std::bad_alloc&) {
    return PM_ERR_NOMEM;
  }
  const uint32_t need = PM_TRACK_PREDICTED | PM_TRACK_MATCHED;
  for (int i = 0; i < n; ++i) {
    const pm_track& k = tracks[i];
    if ((k.flags & (need | PM_TRACK_FAIL_SAD | PM_TRACK_FAIL_GAP)) != need) continue;
    const double Z = fxb / (double)k.disp;  // pm_backproject's point before its rounding
    pts.push_back(Point{(((double)k.x - c.cx) * Z) / c.fx, (((double)k.y - c.cy) * Z) / c.fy, Z, (double)k.x_new, (double)k.y_new});
  }
  double R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = start.R[i];
  for (int i = 0; i < 3; ++i) t[i] = start.t[i];
  bool failed = false;
  int done = 0;
  for (int it = 0; it < options->iterations; ++it) {
    double H[6][6] = {}, g[6] = {};  // from +0.0, in track order
    for (const Point& p : pts) {
      const Residual r = residual(c, R, t, p);
      if (!r.used) continue;
      const double w = r.e <= options->huber_px ? 1.0 : options->huber_px / r.e;
      const double A = c.fx * r.iz, C = -((c.fx * r.a) * r.iz);
      const double B = c.fy * r.iz, D = -((c.fy * r.b) * r.iz);
      const double Ju[6] = {C * r.Qy, (A * r.Qz) - (C * r.Qx), -(A * r.Qy), A, 0.0, C};
      const double Jv[6] = {(D * r.Qy) - (B * r.Qz), -(D * r.Qx), B * r.Qx, 0.0, B, D};
      for (int i = 0; i < 6; ++i) {
        for (int j = i; j < 6; ++j) H[i][j] = H[i][j] + (w * ((Ju[i] * Ju[j]) + (Jv[i] * Jv[j])));
        g[i] = g[i] + (w * ((Ju[i] * r.ru) + (Jv[i] * r.rv)));
      }
    }
    double delta[6];
    if (!pm_host::ldlt_solve(H, g, delta)) {
      failed = true;
      break;
    }
    pm_host::cayley_update(R, t, delta);
    ++done;
    double biggest = 0.0;
    for (double v : delta) biggest = std::fabs(v) > biggest ? std::fabs(v) : biggest;
    if (biggest < options->epsilon) break;
  }
  int n_used = 0, n_in = 0;
  double sum = 0.0;
  for (const Point& p : pts) {
    const Residual r = residual(c, R, t, p);
    if (!r.used) continue;
    ++n_used;
    if (r.e <= options->inlier_px) {
      ++n_in;
      sum = sum + r.e2;
    }
  }
  const bool valid = !failed && n_in >= options->min_inliers;
  if (out) {
    for (int i = 0; i < 9; ++i) out->R[i] = valid ? R[i] : start.R[i];
    for (int i = 0; i < 3; ++i) out->t[i] = valid ? t[i] : start.t[i];
  }
  if (info) {
    info->valid = valid ? 1 : 0;
    info->n_tracks = (int)pts.size();
    info->n_used = n_used;
    info->n_inliers = n_in;
    info->iterations = done;
    info->rms_px = n_in ? std::sqrt(sum / (double)n_in) : 0.0;
  }
  return PM_OK;
}
