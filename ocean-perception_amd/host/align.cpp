// align.cpp -- pm_align_step, pm_motion_compose and pm_align_sums_blend (include/pm/imaging.h): the host half of
// pm_align_disparity and pm_align_color_disparity, in binary64.
// Held to tests/align_ref.py::step and ::compose BIT FOR BIT: the solve and the update are motion_solve.hpp's, shared with
// pm_solve_motion; every operation is one rounding; this unit is compiled with -ffp-contract=off.  It sees the C ABI only, no
// handle and no HIP header.
#include "motion_solve.hpp"
#include "pm/imaging.h"

extern "C" int pm_align_step(const pm_align_sums* sums, const pm_motion* in, pm_motion* out, double delta[6], int* factorised) {
  if (!sums || !out) return PM_ERR_INVALID_ARG;
  double H[6][6] = {}, d[6] = {0, 0, 0, 0, 0, 0};
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) H[i][j] = sums->H[k++];  // the solve reads the upper triangle
  pm_motion m = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
  if (in) m = *in;
  const bool ok = pm_host::ldlt_solve(H, sums->g, d);
  if (ok)
    pm_host::cayley_update(m.R, m.t, d);
  else
    for (double& v : d) v = 0.0;
  *out = m;
  for (int i = 0; delta && i < 6; ++i) delta[i] = d[i];
  if (factorised) *factorised = ok ? 1 : 0;
  return PM_OK;
}

extern "C" int pm_motion_compose(const pm_motion* a, const pm_motion* b, pm_motion* out) {
  if (!a || !b || !out) return PM_ERR_INVALID_ARG;
  pm_motion m;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      m.R[3 * i + j] = ((a->R[3 * i] * b->R[j]) + (a->R[3 * i + 1] * b->R[3 + j])) + (a->R[3 * i + 2] * b->R[6 + j]);
    m.t[i] = (((a->R[3 * i] * b->t[0]) + (a->R[3 * i + 1] * b->t[1])) + (a->R[3 * i + 2] * b->t[2])) + a->t[i];
  }
  *out = m;
  return PM_OK;
}

// Held to tests/align_photo_ref.py::blend BIT FOR BIT: l2 once, then one multiplication and one addition per double.
extern "C" int pm_align_sums_blend(const pm_align_sums* geo, const pm_align_sums* photo, double lambda, pm_align_sums* out) {
  if (!geo || !photo || !out || !(lambda >= 0.0) || !(lambda - lambda == 0.0)) return PM_ERR_INVALID_ARG;
  const double l2 = lambda * lambda;
  pm_align_sums s;
  for (int i = 0; i < 21; ++i) s.H[i] = geo->H[i] + (l2 * photo->H[i]);
  for (int i = 0; i < 6; ++i) s.g[i] = geo->g[i] + (l2 * photo->g[i]);
  s.rr = geo->rr + (l2 * photo->rr);
  s.n_model = geo->n_model + photo->n_model, s.n_gate = geo->n_gate + photo->n_gate, s.n_used = geo->n_used + photo->n_used;
  s.pad = 0;
  *out = s;  // out may alias either input
  return PM_OK;
}
