"""The definition of pm_filter_consistency (include/pm/imaging.h) in numpy: the CURRENT left disparity map judged by n
earlier left maps of the same size and rectified camera, each reached through the rigid motion between the two left cameras.
The kernel is held to it with tolerance 0, like tests/reproject_ref.py: every operation below is ONE rounding in the format
named, with the parentheses as written (numpy's element-wise +, -, *, / and rint are IEEE operations).

camera: (fx, fy, cx, cy, baseline), binary64.  motions[k] = (R[9] row-major, t[3]), binary64: a point X of the CURRENT left
camera's frame is R X + t in source k's left camera frame -- reproject_ref.relative_motion(T_world_cur, T_world_src_k).
  valid     a current pixel is valid iff d = D(y, x) > 0 (binary32): not for 0, -0.0, negatives and NaN; +inf is valid.
  project   into source k, EXACTLY the splat arithmetic of reproject_ref.splat_left with min_disp = 0 and max_disp = 0.  In
            binary64, fxB = fx * baseline (once):  Z = fxB / (double)d;  X = (((double)x - cx) * Z) / fx;
            Y = (((double)y - cy) * Z) / fy;  Xn = (((R0*X) + (R1*Y)) + (R2*Z)) + t0;  Yn with R3..R5, t1;  Zn with R6..R8, t2;
            dropped unless Zn > 0;  dp = (float)(fxB / Zn), dropped unless dp > 0 and finite;  u = (fx * (Xn / Zn)) + cx;
            v = (fy * (Yn / Zn)) + cy;  dropped unless |u| < 2^30 and |v| < 2^30;  iu = rint(u), iv = rint(v) (half to even);
            dropped unless 0 <= iu < cols and 0 <= iv < rows.  A dropped pixel has class UNSEEN.
  tap       the window dy = -radius..radius (outer), dx = -radius..radius (inner) around (iu, iv); a tap COUNTS iff it lies
            inside the image and ds = D_k(iv + dy, iu + dx) > 0.  e = (double)ds - (double)dp.  The chosen tap is the FIRST
            with the smallest fabs(e): a later one replaces it only with a strictly smaller value (ds = +inf gives e = +inf and
            loses against any finite one).  No counting tap: UNSEEN.
  class     md = (double)max_diff:  fabs(e) <= md CONSISTENT (1);  e > md OCCLUDED (2);  e < -md CONFLICT (3);  UNSEEN 0.
  pixel     n_cons, n_conf = sources of class 1, 3.  S = binary64 sum from +0.0 over k in order of fabs(e_k), CONSISTENT
            sources only.  KEPT iff valid and n_cons >= min_consistent and n_conf <= max_conflicts.
  outputs   out: a valid pixel that is not KEPT becomes +0.0f, every other pixel keeps its input BITS;  classes: uint16, the
            class of source k in bits 2k, 2k + 1, 0 for an invalid pixel;  residual: (float)(S / (double)n_cons), +0.0 where
            n_cons == 0 or the pixel is invalid;  counts: int32 [valid pixels, kept pixels].
"""
import numpy as np

UNSEEN, CONSISTENT, OCCLUDED, CONFLICT = 0, 1, 2, 3
MAX_SOURCES = 8


def project(disp, camera, R, t):
    """The current map into one source -> (seen [rows][cols] bool, iu, iv int64 (0 where not seen), dp float32)."""
    fx, fy, cx, cy, baseline = (np.float64(v) for v in camera)
    R = np.asarray(R, np.float64).ravel()
    t = np.asarray(t, np.float64).ravel()
    disp = np.asarray(disp, np.float32)
    rows, cols = disp.shape
    fxb = fx * baseline
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        ok = disp > np.float32(0)  # false for NaN
        d = np.where(ok, disp, np.float32(1)).astype(np.float64)
        Z = fxb / d
        X = ((x - cx) * Z) / fx
        Y = ((y - cy) * Z) / fy
        Xn = (((R[0] * X) + (R[1] * Y)) + (R[2] * Z)) + t[0]
        Yn = (((R[3] * X) + (R[4] * Y)) + (R[5] * Z)) + t[1]
        Zn = (((R[6] * X) + (R[7] * Y)) + (R[8] * Z)) + t[2]
        ok &= Zn > 0
        dp = (fxb / Zn).astype(np.float32)
        ok &= (dp > np.float32(0)) & np.isfinite(dp)
        u = (fx * (Xn / Zn)) + cx
        v = (fy * (Yn / Zn)) + cy
        ok &= (np.abs(u) < 2.0 ** 30) & (np.abs(v) < 2.0 ** 30)
        iu, iv = np.rint(u), np.rint(v)
        ok &= (iu >= 0) & (iu < cols) & (iv >= 0) & (iv < rows)
    iu = np.where(ok, iu, 0).astype(np.int64)
    iv = np.where(ok, iv, 0).astype(np.int64)
    return ok, iu, iv, dp


def classify(disp, source, camera, R, t, max_diff, radius):
    """One source -> (class [rows][cols] uint8, fabs(e) of the chosen tap float64 (0 where UNSEEN), e float64)."""
    source = np.asarray(source, np.float32)
    rows, cols = source.shape
    seen, iu, iv, dp = project(disp, camera, R, t)
    dp64 = dp.astype(np.float64)
    found = np.zeros((rows, cols), bool)
    best = np.zeros((rows, cols), np.float64)
    e = np.zeros((rows, cols), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                yy, xx = iv + dy, iu + dx
                inside = seen & (yy >= 0) & (yy < rows) & (xx >= 0) & (xx < cols)
                ds = np.where(inside, source[np.clip(yy, 0, rows - 1), np.clip(xx, 0, cols - 1)], np.float32(0))
                ek = ds.astype(np.float64) - dp64
                ak = np.abs(ek)
                take = (ds > np.float32(0)) & (~found | (ak < best))
                e = np.where(take, ek, e)
                best = np.where(take, ak, best)
                found |= take
        md = np.float64(np.float32(max_diff))
        cls = np.where(best <= md, CONSISTENT, np.where(e > md, OCCLUDED, CONFLICT))
    cls = np.where(found, cls, UNSEEN).astype(np.uint8)
    return cls, np.where(found, best, 0.0), np.where(found, e, 0.0)


def filter_consistency(disp, sources, camera, motions, max_diff=1.0, radius=1, min_consistent=1, max_conflicts=0):
    """-> dict(out float32, classes uint16, residual float32 [rows][cols]; counts int32[2]; per_source: uint8 [n][rows][cols],
    the class of every source, for the tests to look at)."""
    disp = np.asarray(disp, np.float32)
    n = len(sources)
    assert 1 <= n <= MAX_SOURCES and len(motions) == n
    rows, cols = disp.shape
    with np.errstate(invalid="ignore"):
        valid = disp > np.float32(0)
    classes = np.zeros((rows, cols), np.uint16)
    n_cons = np.zeros((rows, cols), np.int32)
    n_conf = np.zeros((rows, cols), np.int32)
    S = np.zeros((rows, cols), np.float64)
    per_source = np.zeros((n, rows, cols), np.uint8)
    for k in range(n):
        cls, abs_e, _ = classify(disp, sources[k], camera, motions[k][0], motions[k][1], max_diff, radius)
        per_source[k] = cls
        classes |= cls.astype(np.uint16) << np.uint16(2 * k)
        n_cons += cls == CONSISTENT
        n_conf += cls == CONFLICT
        S = np.where(cls == CONSISTENT, S + abs_e, S)
    kept = valid & (n_cons >= min_consistent) & (n_conf <= max_conflicts)
    out = disp.copy()
    out[valid & ~kept] = np.float32(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        residual = np.where(n_cons > 0, (S / np.maximum(n_cons, 1).astype(np.float64)).astype(np.float32), np.float32(0))
    counts = np.array([valid.sum(), kept.sum()], np.int32)
    return dict(out=out, classes=classes, residual=residual.astype(np.float32), counts=counts, per_source=per_source, kept=kept,
                valid=valid)
