// motion_solve.hpp -- the 6x6 solve and the pose update that pm_solve_motion (motion.cpp) and pm_align_step (align.cpp) share: ONE
// statement of each, so that the two Gauss-Newton loops cannot drift apart.  Internal to the host units; every operation is one
// binary64 rounding, parentheses and the order of every sum as tests/motion_ref.py writes them (the units that include it are
// compiled with -ffp-contract=off).  No HIP header, no handle.
#pragma once

namespace pm_host {

// H delta = -g by LDL^T without pivoting, k ascending in every inner sum; false where a pivot is not > 0
inline bool ldlt_solve(const double H[6][6], const double g[6], double delta[6]) {
  double L[6][6] = {}, D[6] = {};
  for (int j = 0; j < 6; ++j) {
    double s = H[j][j];
    for (int k = 0; k < j; ++k) s = s - ((L[j][k] * L[j][k]) * D[k]);
    if (!(s > 0.0)) return false;
    D[j] = s;
    for (int i = j + 1; i < 6; ++i) {
      s = H[j][i];
      for (int k = 0; k < j; ++k) s = s - ((L[i][k] * L[j][k]) * D[k]);
      L[i][j] = s / D[j];
    }
  }
  double y[6], z[6];
  for (int i = 0; i < 6; ++i) {
    double s = -g[i];
    for (int k = 0; k < i; ++k) s = s - (L[i][k] * y[k]);
    y[i] = s;
  }
  for (int i = 0; i < 6; ++i) z[i] = y[i] / D[i];
  for (int i = 5; i >= 0; --i) {
    double s = z[i];
    for (int k = i + 1; k < 6; ++k) s = s - (L[k][i] * delta[k]);
    delta[i] = s;
  }
  return true;
}

// a = omega / 2; dR = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a); R <- dR R; t <- dR t + upsilon
inline void cayley_update(double R[9], double t[3], const double delta[6]) {
  const double a0 = 0.5 * delta[0], a1 = 0.5 * delta[1], a2 = 0.5 * delta[2];
  const double s = ((a0 * a0) + (a1 * a1)) + (a2 * a2);
  const double c = 1.0 - s, den = 1.0 + s;
  const double dR[3][3] = {
      {(c + ((2 * a0) * a0)) / den, (((2 * a0) * a1) - (2 * a2)) / den, (((2 * a0) * a2) + (2 * a1)) / den},
      {(((2 * a1) * a0) + (2 * a2)) / den, (c + ((2 * a1) * a1)) / den, (((2 * a1) * a2) - (2 * a0)) / den},
      {(((2 * a2) * a0) - (2 * a1)) / den, (((2 * a2) * a1) + (2 * a0)) / den, (c + ((2 * a2) * a2)) / den}};
  double Rn[9], tn[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Rn[3 * i + j] = ((dR[i][0] * R[j]) + (dR[i][1] * R[3 + j])) + (dR[i][2] * R[6 + j]);
    tn[i] = (((dR[i][0] * t[0]) + (dR[i][1] * t[1])) + (dR[i][2] * t[2])) + delta[3 + i];
  }
  for (int i = 0; i < 9; ++i) R[i] = Rn[i];
  for (int i = 0; i < 3; ++i) t[i] = tn[i];
}

}  // namespace pm_host
