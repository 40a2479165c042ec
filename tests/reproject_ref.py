"""The definition of pm_reproject_disparity (include/pm/imaging.h) in numpy: the left disparity map of an OLD frame carried
into the NEW frame's two seed maps through the rigid motion between the two left cameras.  The kernels are held to it with
tolerance 0, like tests/pointcloud_ref.py: every operation below is ONE rounding in the format named, with the parentheses
as written (numpy's element-wise +, -, *, / and rint are IEEE operations).

camera: (fx, fy, cx, cy, baseline) of the rectified left view, binary64.  R[9] (row-major), t[3]: binary64; a point X of the
old left camera's frame is R X + t in the new left camera's frame.
  splat   a source pixel (x, y) with value d takes part iff d > 0 and d >= min_disp (binary32; never for NaN).  In binary64,
          fxB = fx * baseline (once):  Z = fxB / (double)d;  X = (((double)x - cx) * Z) / fx;  Y = (((double)y - cy) * Z) / fy;
          Xn = (((R0*X) + (R1*Y)) + (R2*Z)) + t0;  Yn with R3..R5, t1;  Zn with R6..R8, t2;  dropped unless Zn > 0;
          dn = (float)(fxB / Zn), dropped unless dn > 0 and finite, and unless dn <= max_disp where max_disp != 0;
          u = (fx * (Xn / Zn)) + cx;  v = (fy * (Yn / Zn)) + cy;  dropped unless |u| < 2^30 and |v| < 2^30;
          iu = rint(u), iv = rint(v) (half to even);  dropped unless 0 <= iu < cols and 0 <= iv < rows.
          S(iv, iu) = the binary32 maximum of dn over everything that lands there (the nearest surface wins; all candidates are
          > 0 and finite, so the unsigned order of their bits is their order); +0.0 where nothing lands.
  close   C(y, x) = S(y, x) where S(y, x) > 0; elsewhere the maximum of S over the (2r+1)^2 window around it, taps outside the
          image not counting, 0 if no tap is > 0.  r = 0 copies.  A pixel that was hit is never altered.
  right   from the CLOSED left seed C_l: every (x, y) with s = C_l(y, x) > 0 gives q = rint((double)x - (double)s), dropped
          unless 0 <= q < cols;  S_r(y, q) = the maximum of s over its contributors, else +0.0: a map in right-image
          coordinates, the convention pm_mask_occlusions reads.  Then the same close with the same r.
  counts  [pixels > 0 of C_l, pixels > 0 of C_r].
"""
import numpy as np


def _raise_to_max(rows, cols, ok, iy, ix, values):
    """The map of the binary32 maximum of `values` per target pixel, +0.0 elsewhere, and the number of arrivals per pixel."""
    at = iy[ok].astype(np.int64) * cols + ix[ok].astype(np.int64)
    out = np.zeros(rows * cols, np.uint32)
    np.maximum.at(out, at, np.ascontiguousarray(values[ok]).view(np.uint32))  # > 0 and finite: bit order is float order
    hits = np.zeros(rows * cols, np.int32)
    np.add.at(hits, at, 1)
    return out.view(np.float32).reshape(rows, cols), hits.reshape(rows, cols)


def splat_left(disp, camera, R, t, min_disp=0.0, max_disp=0.0):
    """Stage 1 -> (S_l [rows][cols] float32, arrivals per pixel [rows][cols] int32)."""
    fx, fy, cx, cy, baseline = (np.float64(v) for v in camera)
    R = np.asarray(R, np.float64).ravel()
    t = np.asarray(t, np.float64).ravel()
    disp = np.asarray(disp, np.float32)
    rows, cols = disp.shape
    fxb = fx * baseline
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        ok = (disp > np.float32(0)) & (disp >= np.float32(min_disp))  # false for NaN
        d = np.where(ok, disp, np.float32(1)).astype(np.float64)
        Z = fxb / d
        X = ((x - cx) * Z) / fx
        Y = ((y - cy) * Z) / fy
        Xn = (((R[0] * X) + (R[1] * Y)) + (R[2] * Z)) + t[0]
        Yn = (((R[3] * X) + (R[4] * Y)) + (R[5] * Z)) + t[1]
        Zn = (((R[6] * X) + (R[7] * Y)) + (R[8] * Z)) + t[2]
        ok &= Zn > 0
        dn = (fxb / Zn).astype(np.float32)
        ok &= (dn > np.float32(0)) & np.isfinite(dn)
        if np.float32(max_disp) != np.float32(0):
            ok &= dn <= np.float32(max_disp)
        u = (fx * (Xn / Zn)) + cx
        v = (fy * (Yn / Zn)) + cy
        ok &= (np.abs(u) < 2.0 ** 30) & (np.abs(v) < 2.0 ** 30)
        iu, iv = np.rint(u), np.rint(v)
        ok &= (iu >= 0) & (iu < cols) & (iv >= 0) & (iv < rows)
    return _raise_to_max(rows, cols, ok, iv, iu, dn)


def close(S, r):
    """Stage 2."""
    S = np.asarray(S, np.float32)
    rows, cols = S.shape
    with np.errstate(invalid="ignore"):
        hit = S > np.float32(0)
    taps = np.pad(np.where(hit, S, np.float32(0)), r)
    best = np.zeros((rows, cols), np.float32)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            best = np.maximum(best, taps[dy:dy + rows, dx:dx + cols])
    return np.where(hit, S, best).astype(np.float32)


def splat_right(closed_l):
    """Stage 3 in front of its close -> (S_r, arrivals per pixel)."""
    C = np.asarray(closed_l, np.float32)
    rows, cols = C.shape
    x = np.broadcast_to(np.arange(cols, dtype=np.float64)[None, :], (rows, cols))
    y = np.broadcast_to(np.arange(rows, dtype=np.float64)[:, None], (rows, cols))
    with np.errstate(invalid="ignore"):
        ok = C > np.float32(0)
        q = np.rint(x - C.astype(np.float64))
        ok = ok & (q >= 0) & (q < cols)
    return _raise_to_max(rows, cols, ok, y, q, C)


def reproject(disp, camera, R, t, min_disp=0.0, max_disp=0.0, close_radius=1):
    """-> dict(seed_l, seed_r: what pm_reproject_disparity writes; counts: int32[2]; splat_l, splat_r: the maps in front of
    the close; hits_l, hits_r: arrivals per pixel, > 1 where surfaces collided)."""
    splat_l, hits_l = splat_left(disp, camera, R, t, min_disp, max_disp)
    seed_l = close(splat_l, close_radius)
    splat_r, hits_r = splat_right(seed_l)
    seed_r = close(splat_r, close_radius)
    counts = np.array([(seed_l > 0).sum(), (seed_r > 0).sum()], np.int32)
    return dict(seed_l=seed_l, seed_r=seed_r, counts=counts, splat_l=splat_l, splat_r=splat_r, hits_l=hits_l, hits_r=hits_r)


def relative_motion(T_world_old, T_world_new):
    """T_new_old = T_world_new^-1 * T_world_old for two 4x4 rigid poses (camera to world) -> (R[9], t[3])."""
    A = np.asarray(T_world_old, np.float64).reshape(4, 4)
    B = np.asarray(T_world_new, np.float64).reshape(4, 4)
    Rb, tb = B[:3, :3], B[:3, 3]
    R = Rb.T @ A[:3, :3]
    t = Rb.T @ (A[:3, 3] - tb)
    return R.ravel(), t
