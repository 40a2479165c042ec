"""The definition of pm_disparity_normals (include/pm/imaging.h) in numpy: a windowed, edge-aware least-squares plane per
pixel of a disparity map.  The kernel is held to it with tolerance 0, like tests/pointcloud_ref.py: every operation below is
ONE rounding in the format named, with the parentheses and the ORDER OF THE SUMS as written.

Inputs: disp [rows][cols] binary32; radius r in 1..7; max_diff binary32, finite, >= 0; min_support in 3..(2r+1)^2.
Per pixel (x, y), d0 = disp(y, x):
  not d0 > 0 (0, -0.0, negative, NaN)    no fit, support 0.
  a tap (dx, dy), dx, dy in -r..r, COUNTS iff (x+dx, y+dy) lies in the image, t = disp there is > 0, and
          fabs(e) <= (double)max_diff  with  e = (double)t - (double)d0  in binary64 (a NaN e never counts: d0 = +inf).
  integer sums over the counting taps (exact): n, Sx, Sy, Sxx, Sxy, Syy of 1, dx, dy, dx^2, dx dy, dy^2.
  binary64 sums: per window row dy = -r..r, dx = -r..r left to right, from +0.0:
          R0 = counts ? R0 + e : R0        R1 = counts ? R1 + ((double)dx * e) : R1
      then top to bottom, from +0.0:
          Se = Se + R0        Sxe = Sxe + R1        Sye = Sye + ((double)dy * R0)
  integer cofactors of [[Sxx,Sxy,Sx],[Sxy,Syy,Sy],[Sx,Sy,n]]:
          C00 = Syy*n - Sy*Sy    C01 = Sx*Sy - Sxy*n    C02 = Sxy*Sy - Syy*Sx
          C11 = Sxx*n - Sx*Sx    C12 = Sxy*Sx - Sxx*Sy  C22 = Sxx*Syy - Sxy*Sxy
          det = Sxx*C00 + Sxy*C01 + Sx*C02      (64 bits)
  VALID iff n >= min_support and det > 0 (a collinear or single-pixel support has det == 0 exactly).
  in binary64:  a64 = (((C00*Sxe) + (C01*Sye)) + (C02*Se)) / det,  b64 with (C01, C11, C12),  c64 with (C02, C12, C22).
  a = (float)a64, b = (float)b64, z = (float)((double)d0 + c64): the fitted disparity at the pixel.
Outputs: planes = (a, b, z) where VALID else (0, 0, 0); support = n as uint8, valid or not; normal =
pointcloud_ref.normals(planes, camera): no second statement of the normal arithmetic, and its rules hold ((0, 0, 0) where z
is not > 0 or the length is not finite).
"""
import numpy as np

import pointcloud_ref as PR


def fit(disp, radius, max_diff, min_support):
    """-> planes [3][rows][cols] float32, support [rows][cols] uint8, valid [rows][cols] bool."""
    disp = np.ascontiguousarray(disp, np.float32)
    r = int(radius)
    assert disp.ndim == 2 and 1 <= r <= 7 and 3 <= int(min_support) <= (2 * r + 1) ** 2
    md = np.float64(np.float32(max_diff))
    assert np.isfinite(md) and md >= 0
    rows, cols = disp.shape
    pad = np.zeros((rows + 2 * r, cols + 2 * r), np.float32)  # outside the image: 0.0f, which never counts
    pad[r:r + rows, r:r + cols] = disp
    d0_ok = disp > np.float32(0)  # false for NaN
    d064 = disp.astype(np.float64)
    i64 = lambda: np.zeros((rows, cols), np.int64)
    f64 = lambda: np.zeros((rows, cols), np.float64)
    n, Sx, Sy, Sxx, Sxy, Syy = i64(), i64(), i64(), i64(), i64(), i64()
    Se, Sxe, Sye = f64(), f64(), f64()
    with np.errstate(invalid="ignore", over="ignore"):
        for dy in range(-r, r + 1):
            R0, R1 = f64(), f64()
            for dx in range(-r, r + 1):
                t = pad[r + dy:r + dy + rows, r + dx:r + dx + cols]
                e = t.astype(np.float64) - d064
                counts = d0_ok & (t > np.float32(0)) & (np.abs(e) <= md)
                R0 = np.where(counts, R0 + e, R0)
                R1 = np.where(counts, R1 + (np.float64(dx) * e), R1)
                c = counts.astype(np.int64)
                n += c
                Sx += c * dx
                Sy += c * dy
                Sxx += c * (dx * dx)
                Sxy += c * (dx * dy)
                Syy += c * (dy * dy)
            Se = Se + R0
            Sxe = Sxe + R1
            Sye = Sye + (np.float64(dy) * R0)
        C00 = Syy * n - Sy * Sy
        C01 = Sx * Sy - Sxy * n
        C02 = Sxy * Sy - Syy * Sx
        C11 = Sxx * n - Sx * Sx
        C12 = Sxy * Sx - Sxx * Sy
        C22 = Sxx * Syy - Sxy * Sxy
        det = Sxx * C00 + Sxy * C01 + Sx * C02
        valid = (n >= int(min_support)) & (det > 0)
        den = np.where(valid, det, 1).astype(np.float64)
        F = lambda c: c.astype(np.float64)
        a64 = (((F(C00) * Sxe) + (F(C01) * Sye)) + (F(C02) * Se)) / den
        b64 = (((F(C01) * Sxe) + (F(C11) * Sye)) + (F(C12) * Se)) / den
        c64 = (((F(C02) * Sxe) + (F(C12) * Sye)) + (F(C22) * Se)) / den
        planes = np.stack([a64.astype(np.float32), b64.astype(np.float32), (d064 + c64).astype(np.float32)])
    planes[:, ~valid] = np.float32(0)
    return planes, n.astype(np.uint8), valid


def disparity_normals(disp, camera, radius, max_diff, min_support):
    """-> dict(normals [rows][cols][3] float32, planes [3][rows][cols] float32, support [rows][cols] uint8, valid)."""
    planes, support, valid = fit(disp, radius, max_diff, min_support)
    return {"normals": PR.normals(planes, camera), "planes": planes, "support": support, "valid": valid}
