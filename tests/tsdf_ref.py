"""The definition of pm_tsdf_clear, pm_tsdf_integrate and pm_tsdf_raycast (include/pm/imaging.h) in numpy: a truncated signed
distance volume in the WORLD frame, integrated from left disparity maps with their camera poses (X_cam = R X_world + t) and
raycast back into a left disparity map, with normals, at any pose.  The kernels are held to it with tolerance 0, like
tests/fuse_ref.py: every operation below is ONE rounding in the format named, with the parentheses as written (numpy's
element-wise +, -, *, /, floor, rint and sqrt are IEEE operations).

A volume is (grid, voxels): grid = dict(nx, ny, nz, origin[3], voxel, trunc, max_weight); voxels float32 [nz][ny][nx][2], the
pair being (tsdf, weight) -- the bytes of the device buffer.  camera: (fx, fy, cx, cy, baseline), binary64; fxB = fx * baseline.

  integrate  per voxel (i, j, k):  Xw = origin[0] + ((double)i * voxel), Yw, Zw likewise.  From here reproject_ref.splat_left's
             lines with max_disp = 0:  Xc = (((R0*Xw) + (R1*Yw)) + (R2*Zw)) + t0, Yc, Zc likewise;  dropped unless Zc > 0;
             dropped unless (float)(fxB / Zc) is > 0 and finite;  u = (fx * (Xc / Zc)) + cx, v likewise;  dropped unless
             |u| < 2^30 and |v| < 2^30;  iu = rint(u), iv = rint(v);  dropped outside the image.  What is left is IN VIEW.
             d = D(iv, iu) counts iff d > 0 and d >= min_disp (binary32).  Zm = fxB / (double)d;  dropped if max_range != 0 and
             (float)Zm > max_range.  sdf = Zm - Zc;  dropped if sdf < -trunc.  f = (float)fmin(1.0, sdf / trunc).
             wn = 1.0f or W(iv, iu); it takes part iff it is finite and > 0 (fuse_ref.weight64's rule).
             binary32:  tsdf' = ((tsdf * w) + (f * wn)) / (w + wn);  w' = fminf(w + wn, max_weight).
             A dropped voxel keeps its bits.  counts = [in view, updated].
  raycast    Ri, c = fuse_ref.inverse_motion(R, t).  Per pixel:  dx = ((double)x - cx) / fx;  dy = ((double)y - cy) / fy;
             wd_i = ((Ri[3i]*dx) + (Ri[3i+1]*dy)) + Ri[3i+2].  ds = (double)step * trunc;  s_n = (double)min_range +
             ((double)n * ds) for n = 0, 1, ... while s_n <= (double)max_range.  q_i = ((c_i + (s * wd_i)) - origin[i]) / voxel.
             sample(q): b_i = floor(q_i); fr_i = (float)(q_i - b_i); VALID iff 0 <= b_i <= n_i - 2 on every axis and all eight
             corners have weight > 0 and weight >= min_weight; lerp(a, b, t) = a + (t * (b - a)) in binary32: along x for the
             four (row, slice) pairs (b1, b2), (b1+1, b2), (b1, b2+1), (b1+1, b2+1), then along y within each slice, then
             along z.  HIT: the first n with sample n - 1 VALID, f_prev > 0, sample n VALID, f_cur <= 0:
             s* = s_(n-1) + (ds * ((double)f_prev / ((double)f_prev - (double)f_cur))).  VALID f_prev < 0 then VALID f_cur > 0
             ends the ray.  A sample that is not VALID forgets f_prev.  disp = (float)(fxB / s*), +0.0 without a hit.
             normal: q* at s*; G_i = sample(q* + e_i) - sample(q* - e_i) in binary32; (0, 0, 0) if one of the six is not VALID;
             m_i = ((R[3i]*(double)G0) + (R[3i+1]*(double)G1)) + (R[3i+2]*(double)G2);  n_i = (float)m_i;
             l = sqrtf(((n0*n0) + (n1*n1)) + (n2*n2)); (0, 0, 0) unless l > 0 and finite; n_i / l, negated iff
             ((m0*dx) + (m1*dy)) + m2 > 0.  counts = [pixels hit].
"""
import numpy as np

import fuse_ref as FU

MAX_SAMPLES = 1 << 16


def make_grid(nx, ny, nz, origin, voxel, trunc, max_weight=64.0):
    return dict(nx=int(nx), ny=int(ny), nz=int(nz), origin=tuple(float(v) for v in origin), voxel=float(voxel), trunc=float(trunc),
                max_weight=float(max_weight))


def clear(grid):
    return np.zeros((grid["nz"], grid["ny"], grid["nx"], 2), np.float32)


def voxel_centres(grid):
    """(Xw [1][1][nx], Yw [1][ny][1], Zw [nz][1][1]) in binary64."""
    o = [np.float64(v) for v in grid["origin"]]
    vx = np.float64(grid["voxel"])
    X = o[0] + (np.arange(grid["nx"], dtype=np.float64) * vx)
    Y = o[1] + (np.arange(grid["ny"], dtype=np.float64) * vx)
    Z = o[2] + (np.arange(grid["nz"], dtype=np.float64) * vx)
    return X[None, None, :], Y[None, :, None], Z[:, None, None]


def project(X, Y, Z, camera, R, t, rows, cols):
    """reproject_ref.splat_left from its motion line on, max_disp = 0 -> (in view, iu, iv int64 (0 where dropped), Zc)."""
    fx, fy, cx, cy, baseline = (np.float64(v) for v in camera)
    R = np.asarray(R, np.float64).ravel()
    t = np.asarray(t, np.float64).ravel()
    fxb = fx * baseline
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        Xn = (((R[0] * X) + (R[1] * Y)) + (R[2] * Z)) + t[0]
        Yn = (((R[3] * X) + (R[4] * Y)) + (R[5] * Z)) + t[1]
        Zn = (((R[6] * X) + (R[7] * Y)) + (R[8] * Z)) + t[2]
        ok = Zn > 0
        dn = (fxb / Zn).astype(np.float32)
        ok &= (dn > np.float32(0)) & np.isfinite(dn)
        u = (fx * (Xn / Zn)) + cx
        v = (fy * (Yn / Zn)) + cy
        ok &= (np.abs(u) < 2.0 ** 30) & (np.abs(v) < 2.0 ** 30)
        iu, iv = np.rint(u), np.rint(v)
        ok &= (iu >= 0) & (iu < cols) & (iv >= 0) & (iv < rows)
    iu = np.where(ok, iu, 0).astype(np.int64)
    iv = np.where(ok, iv, 0).astype(np.int64)
    return ok, iu, iv, Zn


def integrate(grid, voxels, disp, camera, R, t, weight=None, min_disp=0.0, max_range=0.0):
    """-> dict(voxels: the new volume; counts int32[2]; in_view, updated: bool [nz][ny][nx]); `voxels` is left unchanged."""
    voxels = np.asarray(voxels, np.float32)
    disp = np.asarray(disp, np.float32)
    rows, cols = disp.shape
    fx, baseline = np.float64(camera[0]), np.float64(camera[4])
    fxb = fx * baseline
    trunc = np.float64(grid["trunc"])
    X, Y, Z = voxel_centres(grid)
    seen, iu, iv, Zc = project(X, Y, Z, camera, R, t, rows, cols)
    shape = voxels.shape[:3]
    seen, iu, iv, Zc = (np.broadcast_to(a, shape) for a in (seen, iu, iv, Zc))
    d = disp[iv, iu]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        obs = seen & (d > np.float32(0)) & (d >= np.float32(min_disp))
        Zm = fxb / np.where(obs, d, np.float32(1)).astype(np.float64)
        if np.float32(max_range) != np.float32(0):
            obs = obs & ~(Zm.astype(np.float32) > np.float32(max_range))
        sdf = Zm - Zc
        obs = obs & ~(sdf < -trunc)
        f = np.minimum(np.float64(1.0), sdf / trunc).astype(np.float32)
        if weight is not None:
            wn = np.asarray(weight, np.float32)[iv, iu]
            obs = obs & (FU.weight64(wn) > 0)
        else:
            wn = np.ones(shape, np.float32)
        wn = np.where(obs, wn, np.float32(1))
        f = np.where(obs, f, np.float32(0))
        T, W = voxels[..., 0], voxels[..., 1]
        Tn = ((T * W) + (f * wn)) / (W + wn)
        Wn = np.minimum(W + wn, np.float32(grid["max_weight"]))
    out = voxels.copy()
    out[..., 0] = np.where(obs, Tn, T)
    out[..., 1] = np.where(obs, Wn, W)
    # (np.where copies values: a kept voxel keeps its bits, NaN payloads included, because it is taken from `voxels`)
    keep = ~obs
    out.view(np.uint32)[keep] = voxels.view(np.uint32)[keep]
    return dict(voxels=out, counts=np.array([seen.sum(), obs.sum()], np.int32), in_view=seen.copy(), updated=obs)


def sample_count(min_range, max_range, step, trunc):
    """The number of samples of a ray: the n >= 0 with s_n <= max_range."""
    lo, hi = np.float64(np.float32(min_range)), np.float64(np.float32(max_range))
    ds = np.float64(np.float32(step)) * np.float64(trunc)
    est = (hi - lo) / ds
    assert ds > 0 and 0 <= est < MAX_SAMPLES - 2
    n = int(est) + 1
    while lo + (np.float64(n) * ds) <= hi:
        n += 1
    while n > 0 and not (lo + (np.float64(n - 1) * ds) <= hi):
        n -= 1
    return n


def _lerp(a, b, t):
    return a + (t * (b - a))


def sample(grid, voxels, min_weight, q0, q1, q2):
    """The trilinear value at grid coordinates (q0, q1, q2), binary64 arrays -> (VALID, value float32; 0 where outside)."""
    nx, ny, nz = grid["nx"], grid["ny"], grid["nz"]
    mw = np.float32(min_weight)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        b0, b1, b2 = np.floor(q0), np.floor(q1), np.floor(q2)
        f0, f1, f2 = (q0 - b0).astype(np.float32), (q1 - b1).astype(np.float32), (q2 - b2).astype(np.float32)
        inside = (b0 >= 0) & (b0 <= nx - 2) & (b1 >= 0) & (b1 <= ny - 2) & (b2 >= 0) & (b2 <= nz - 2)
        i0 = np.where(inside, b0, 0).astype(np.int64)
        i1 = np.where(inside, b1, 0).astype(np.int64)
        i2 = np.where(inside, b2, 0).astype(np.int64)
        j0, j1, j2 = np.minimum(i0 + 1, nx - 1), np.minimum(i1 + 1, ny - 1), np.minimum(i2 + 1, nz - 1)
        part = inside.copy()
        corner = {}
        for dz, kz in ((0, i2), (1, j2)):
            for dy, ky in ((0, i1), (1, j1)):
                for dx, kx in ((0, i0), (1, j0)):
                    rec = voxels[kz, ky, kx]
                    corner[dx, dy, dz] = rec[..., 0]
                    part &= (rec[..., 1] > np.float32(0)) & (rec[..., 1] >= mw)
        x00 = _lerp(corner[0, 0, 0], corner[1, 0, 0], f0)
        x10 = _lerp(corner[0, 1, 0], corner[1, 1, 0], f0)
        x01 = _lerp(corner[0, 0, 1], corner[1, 0, 1], f0)
        x11 = _lerp(corner[0, 1, 1], corner[1, 1, 1], f0)
        y0 = _lerp(x00, x10, f1)
        y1 = _lerp(x01, x11, f1)
        value = _lerp(y0, y1, f2)
    return part, np.where(inside, value, np.float32(0)).astype(np.float32)


def raycast(grid, voxels, camera, R, t, rows, cols, min_range=0.1, max_range=10.0, step=0.5, min_weight=0.0):
    """-> dict(disp float32 [rows][cols], normals float32 [rows][cols][3], counts int32[1], hit bool, samples: the rays' n)."""
    voxels = np.asarray(voxels, np.float32)
    fx, fy, cx, cy, baseline = (np.float64(v) for v in camera)
    fxb = fx * baseline
    R = np.asarray(R, np.float64).ravel()
    Ri, c = FU.inverse_motion(R, t)
    o = [np.float64(v) for v in grid["origin"]]
    vx = np.float64(grid["voxel"])
    lo = np.float64(np.float32(min_range))
    ds = np.float64(np.float32(step)) * np.float64(grid["trunc"])
    n_samples = sample_count(min_range, max_range, step, grid["trunc"])
    x = np.broadcast_to(np.arange(cols, dtype=np.float64)[None, :], (rows, cols))
    y = np.broadcast_to(np.arange(rows, dtype=np.float64)[:, None], (rows, cols))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        dx = (x - cx) / fx
        dy = (y - cy) / fy
        wd = [((Ri[3 * i] * dx) + (Ri[3 * i + 1] * dy)) + Ri[3 * i + 2] for i in range(3)]

        def point(s):
            return [((c[i] + (s * wd[i])) - o[i]) / vx for i in range(3)]

        have_prev = np.zeros((rows, cols), bool)
        f_prev = np.zeros((rows, cols), np.float32)
        done = np.zeros((rows, cols), bool)
        hit = np.zeros((rows, cols), bool)
        s_hit = np.ones((rows, cols), np.float64)
        for n in range(n_samples):
            if done.all():
                break
            s = lo + (np.float64(n) * ds)
            valid, f_cur = sample(grid, voxels, min_weight, *point(s))
            live = ~done
            front = live & valid & have_prev & (f_prev > np.float32(0)) & (f_cur <= np.float32(0))
            s_prev = lo + (np.float64(n - 1) * ds)
            fp, fc = f_prev.astype(np.float64), f_cur.astype(np.float64)
            s_new = s_prev + (ds * (fp / (fp - fc)))
            s_hit = np.where(front, s_new, s_hit)
            hit |= front
            back = live & ~front & valid & have_prev & (f_prev < np.float32(0)) & (f_cur > np.float32(0))
            done |= front | back
            have_prev = valid
            f_prev = f_cur
        disp = np.where(hit, (fxb / s_hit).astype(np.float32), np.float32(0)).astype(np.float32)
        q = point(s_hit)
        G, all_six = [], hit.copy()
        for i in range(3):
            qp, qm = list(q), list(q)
            qp[i] = q[i] + 1.0
            qm[i] = q[i] - 1.0
            okp, vp = sample(grid, voxels, min_weight, *qp)
            okm, vm = sample(grid, voxels, min_weight, *qm)
            all_six &= okp & okm
            G.append((vp - vm).astype(np.float64))
        m = [((R[3 * i] * G[0]) + (R[3 * i + 1] * G[1])) + (R[3 * i + 2] * G[2]) for i in range(3)]
        nf = [v.astype(np.float32) for v in m]
        ss = ((nf[0] * nf[0]) + (nf[1] * nf[1])) + (nf[2] * nf[2])
        l = np.sqrt(ss)
        ok = all_six & (l > np.float32(0)) & np.isfinite(l)
        q1 = np.where(ok, l, np.float32(1))
        away = (((m[0] * dx) + (m[1] * dy)) + m[2]) > 0
        normals = np.stack([np.where(ok, np.where(away, -(v / q1), v / q1), np.float32(0)) for v in nf], axis=-1).astype(np.float32)
    return dict(disp=disp, normals=normals, counts=np.array([hit.sum()], np.int32), hit=hit, samples=n_samples)
