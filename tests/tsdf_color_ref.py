"""The definition of pm_tsdf_color_clear, pm_tsdf_integrate_color, pm_tsdf_color_map and pm_tsdf_color_points
(include/pm/imaging.h) in numpy: a colour volume beside the distance volume of tests/tsdf_ref.py, integrated with it from left
disparity maps and their images, and read back at the pixels of a left map at a pose or at world-frame points.  The kernels are
held to it with tolerance 0: every operation below is ONE rounding in the format named, with the parentheses as written.

A colour volume is float32 [nz][ny][nx][4], the four being (b, g, r, weight) -- the bytes of the device buffer; weight == 0: never
coloured.  grid, voxels, camera: tests/tsdf_ref.py's.

  integrate  the distance volume and counts [0], [1]: tsdf_ref.integrate itself.  Per voxel that it UPDATED, with its (iu, iv), Zc,
             d = D(iv, iu), Zm = fxB / (double)d and sdf = Zm - Zc:  bandw = (double)(float)band * trunc;  COLOURED iff
             sdf <= bandw and sdf >= -bandw and, with a float image, the three channels of pixel (iv, iu) are finite.
             p_c = (float)bgr8[iv][iu][c] or bgr[iv][iu][c];  wn = 1.0f or W(iv, iu);  w the colour record's weight.  binary32:
             C'_c = ((C_c * w) + (p_c * wn)) / (w + wn);  w' = fminf(w + wn, max_weight).  Every other record keeps its bits.
             counts = [in view, updated, coloured].
  sample     at grid coordinates q (binary64): dropped unless |q_i| < 2^30 on every axis.  lo_i = floor(q_i);
             fr_i = (float)(q_i - lo_i).  Corner c = 0..7 (bit 0 x, bit 1 y, bit 2 z) sits at lo + bits and has the binary32
             weight tw = (wx * wy) * wz, w = 1.0f - fr on a 0 bit and fr on a 1 bit.  It TAKES PART iff it lies inside the grid,
             its colour weight is > 0 and >= min_weight and its three channels are finite.  binary32, from 0, ascending c, the
             others skipped:  den = den + tw;  num_c = num_c + (tw * C_c).  COLOURED iff den > 0;  value_c = num_c / den.
  outputs    bgr = value_c;  bgr8 = (uint8)fminf(fmaxf(rintf(value_c * byte_scale), 0), 255);  zeros where not coloured;
             counts = [coloured].
  map        pixel (x, y) counts iff d = D(y, x) > 0;  s = fxB / (double)d;  tsdf_ref.raycast's Ri, c, dx, dy, wd_i;
             q_i = ((c_i + (s * wd_i)) - origin[i]) / voxel.
  points     q_i = ((double)P_i - origin[i]) / voxel, for the first `limit` points; the others' outputs keep their bytes.
"""
import numpy as np

import fuse_ref as FU
import tsdf_ref as TR

_QUIET = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


def clear(grid):
    return np.zeros((grid["nz"], grid["ny"], grid["nx"], 4), np.float32)


def integrate(grid, voxels, colors, disp, image, camera, R, t, weight=None, min_disp=0.0, max_range=0.0, band=1.0):
    """image: uint8 or float32 [rows][cols][3].  -> dict(voxels, colors: the new volumes; counts int32[3]; updated, colored: bool
    [nz][ny][nx]; sdf: binary64 [nz][ny][nx], meaningful where updated); the inputs are left unchanged."""
    colors = np.asarray(colors, np.float32)
    disp = np.asarray(disp, np.float32)
    image = np.asarray(image)
    assert image.dtype in (np.uint8, np.float32) and image.shape == disp.shape + (3,)
    rows, cols = disp.shape
    out = TR.integrate(grid, voxels, disp, camera, R, t, weight, min_disp, max_range)
    up = out["updated"]
    shape = up.shape
    fxb = np.float64(camera[0]) * np.float64(camera[4])
    X, Y, Z = TR.voxel_centres(grid)
    _, iu, iv, Zc = TR.project(X, Y, Z, camera, R, t, rows, cols)
    iu, iv, Zc = (np.broadcast_to(a, shape) for a in (iu, iv, Zc))
    with np.errstate(**_QUIET):
        d = disp[iv, iu]
        Zm = fxb / np.where(up, d, np.float32(1)).astype(np.float64)
        sdf = Zm - Zc
        bandw = np.float64(np.float32(band)) * np.float64(grid["trunc"])
        col = up & (sdf <= bandw) & (sdf >= -bandw)
        p = image[iv, iu].astype(np.float32)  # [nz][ny][nx][3]
        if image.dtype != np.uint8:
            col = col & np.isfinite(p).all(-1)
        wn = np.asarray(weight, np.float32)[iv, iu] if weight is not None else np.ones(shape, np.float32)
        wn = np.where(col, wn, np.float32(1))
        p = np.where(col[..., None], p, np.float32(0))
        C, W = colors[..., :3], colors[..., 3]
        Cn = ((C * W[..., None]) + (p * wn[..., None])) / (W + wn)[..., None]
        Wn = np.fmin(W + wn, np.float32(grid["max_weight"]))
    new = colors.copy()
    new[..., :3] = Cn
    new[..., 3] = Wn
    keep = ~col
    new.view(np.uint32)[keep] = colors.view(np.uint32)[keep]  # an uncoloured record keeps its bits, NaN payloads included
    counts = np.array([out["counts"][0], out["counts"][1], col.sum()], np.int32)
    return dict(voxels=out["voxels"], colors=new, counts=counts, updated=up, colored=col, sdf=sdf, in_view=out["in_view"])


def sample(grid, colors, min_weight, q0, q1, q2):
    """The normalised trilinear mean at grid coordinates (binary64 arrays of one shape) -> (COLOURED, value float32 [...][3];
    0 where not coloured, den float32, parts: how many corners took part)."""
    colors = np.asarray(colors, np.float32)
    n = (grid["nx"], grid["ny"], grid["nz"])
    mw = np.float32(min_weight)
    q = [np.asarray(v, np.float64) for v in (q0, q1, q2)]
    with np.errstate(**_QUIET):
        ok = (np.abs(q[0]) < 2.0 ** 30) & (np.abs(q[1]) < 2.0 ** 30) & (np.abs(q[2]) < 2.0 ** 30)
        q = [np.where(ok, v, 0.0) for v in q]
        lo = [np.floor(v) for v in q]
        fr = [(v - l).astype(np.float32) for v, l in zip(q, lo)]
        lo = [l.astype(np.int64) for l in lo]
        w = [(np.float32(1) - f, f) for f in fr]
        den = np.zeros(q[0].shape, np.float32)
        num = [np.zeros(q[0].shape, np.float32) for _ in range(3)]
        parts = np.zeros(q[0].shape, np.int32)
        for c in range(8):
            bit = (c & 1, (c >> 1) & 1, c >> 2)
            at = [lo[i] + bit[i] for i in range(3)]
            inside = ok.copy()
            for i in range(3):
                inside &= (at[i] >= 0) & (at[i] < n[i])
            rec = colors[np.clip(at[2], 0, n[2] - 1), np.clip(at[1], 0, n[1] - 1), np.clip(at[0], 0, n[0] - 1)]
            part = inside & (rec[..., 3] > np.float32(0)) & (rec[..., 3] >= mw) & np.isfinite(rec[..., :3]).all(-1)
            tw = (w[0][bit[0]] * w[1][bit[1]]) * w[2][bit[2]]
            den = np.where(part, den + tw, den)
            for k in range(3):
                num[k] = np.where(part, num[k] + (tw * rec[..., k]), num[k])
            parts += part
        colored = den > np.float32(0)
        safe = np.where(colored, den, np.float32(1))
        value = np.stack([np.where(colored, v / safe, np.float32(0)) for v in num], -1).astype(np.float32)
    return colored, value, den, parts


def outputs(colored, value, byte_scale):
    """-> (bgr float32 [...][3], bgr8 uint8 [...][3]) of a sample."""
    with np.errstate(**_QUIET):
        b = np.fmin(np.fmax(np.rint(value * np.float32(byte_scale)), np.float32(0)), np.float32(255))
    b8 = np.where(colored[..., None], b, np.float32(0)).astype(np.uint8)
    return np.where(colored[..., None], value, np.float32(0)).astype(np.float32), b8


def map_coordinates(grid, disp, camera, R, t):
    """-> (counts: bool [rows][cols], q0, q1, q2 binary64 [rows][cols]) of pm_tsdf_color_map's pixels."""
    disp = np.asarray(disp, np.float32)
    rows, cols = disp.shape
    fx, fy, cx, cy, baseline = (np.float64(v) for v in camera)
    fxb = fx * baseline
    Ri, c = FU.inverse_motion(np.asarray(R, np.float64).ravel(), t)
    o = [np.float64(v) for v in grid["origin"]]
    vx = np.float64(grid["voxel"])
    x = np.broadcast_to(np.arange(cols, dtype=np.float64)[None, :], (rows, cols))
    y = np.broadcast_to(np.arange(rows, dtype=np.float64)[:, None], (rows, cols))
    with np.errstate(**_QUIET):
        has = disp > np.float32(0)
        s = fxb / np.where(has, disp, np.float32(1)).astype(np.float64)
        dx = (x - cx) / fx
        dy = (y - cy) / fy
        wd = [((Ri[3 * i] * dx) + (Ri[3 * i + 1] * dy)) + Ri[3 * i + 2] for i in range(3)]
        q = [((c[i] + (s * wd[i])) - o[i]) / vx for i in range(3)]
    return has, q[0], q[1], q[2]


def color_map(grid, colors, disp, camera, R, t, min_weight=0.0, byte_scale=1.0):
    """-> dict(bgr float32 [rows][cols][3], bgr8 uint8 [rows][cols][3], counts int32[1], colored bool [rows][cols])."""
    has, q0, q1, q2 = map_coordinates(grid, disp, camera, R, t)
    colored, value, _, _ = sample(grid, colors, min_weight, q0, q1, q2)
    colored = colored & has
    bgr, bgr8 = outputs(colored, value, byte_scale)
    return dict(bgr=bgr, bgr8=bgr8, counts=np.array([colored.sum()], np.int32), colored=colored)


def point_coordinates(grid, xyz):
    P = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(**_QUIET):
        return [(P[:, i] - np.float64(grid["origin"][i])) / np.float64(grid["voxel"]) for i in range(3)]


def color_points(grid, colors, xyz, min_weight=0.0, byte_scale=1.0, limit=None, bgr=None, bgr8=None):
    """xyz float32 [n][3].  limit: min(n, *d_n), None = n; the outputs behind it are taken from `bgr` / `bgr8` (default zeros).
    -> dict(bgr, bgr8, counts int32[1], colored bool [n], parts int32 [n])."""
    n = np.asarray(xyz).reshape(-1, 3).shape[0]
    m = n if limit is None else max(0, min(n, int(limit)))
    colored, value, _, parts = sample(grid, colors, min_weight, *point_coordinates(grid, xyz))
    colored = colored & (np.arange(n) < m)
    o, o8 = outputs(colored, value, byte_scale)
    out = np.zeros((n, 3), np.float32) if bgr is None else np.array(bgr, np.float32).reshape(n, 3)
    out8 = np.zeros((n, 3), np.uint8) if bgr8 is None else np.array(bgr8, np.uint8).reshape(n, 3)
    out.view(np.uint32)[:m] = o.view(np.uint32)[:m]
    out8[:m] = o8[:m]
    return dict(bgr=out, bgr8=out8, counts=np.array([colored.sum()], np.int32), colored=colored, parts=parts)
