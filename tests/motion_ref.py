"""The definition of pm_track_features, pm_solve_motion and pm_estimate_motion (include/pm/imaging.h) in numpy: the rigid
motion of the left camera between two frames of a sequence, from the old left image, its disparity map and the new left
image.  The kernels and the host solver are held to it with tolerance 0: the tracking half is exact integer arithmetic up to
the prediction, which is pm_reproject_disparity's `splat` arithmetic (tests/reproject_ref.py), and every floating-point
operation below is ONE rounding in the format named, parentheses as written, sums in the order written.

camera: (fx, fy, cx, cy, baseline), binary64; fxB = fx * baseline, formed once.  A motion (R[9] row-major, t[3]) takes a point
X of the OLD left camera's frame to R X + t in the NEW one's: pm_reproject_disparity's convention.
  score     gx, gy: the 3x3 Sobel responses of the old image (int);  Sxx, Syy, Sxy: sums of gx gx, gy gy, gx gy over the 7x7
            window;  score = 16 (Sxx Syy - Sxy Sxy) - (Sxx + Syy)^2 in int64 (Harris with k = 1/16; at most about 4.2e16).
  eligible  m = max(p, 4);  m <= x <= cols - 1 - m, m <= y <= rows - 1 - m;  d = D_old(y, x) finite, > 0, >= min_disp, and
            <= max_disp where max_disp != 0;  score >= min_score.
  select    cell (cx, cy) covers x in [cx cell, min(cols, (cx + 1) cell)) and y likewise;  its feature is the eligible pixel
            of the largest score, a tie going to the smallest y cols + x;  the features are numbered by cell in row-major
            order: the k-th is record k.
  predict   `splat`'s Z, X, Y, Xn, Yn, Zn, u, v;  PREDICTED iff Zn > 0 and |u| < 2^30 and |v| < 2^30;  iu = rint(u),
            iv = rint(v) (half to even), which may lie outside the image.  A record that is not predicted has x_new = y_new = 0,
            sad = second = INT32_MAX and no flag.
  match     candidates (qx, qy) = (iu + ex, iv + ey), ey and ex in -s .. s, row-major; a candidate COUNTS iff its (2p+1)^2
            patch lies inside the new image;  SAD = sum |old(y + dy, x + dx) - new(qy + dy, qx + dx)|;  the best candidate is
            the first of the smallest SAD;  MATCHED iff a candidate counts.  second: the smallest SAD among the counting
            candidates at Chebyshev distance >= 2 from the best, INT32_MAX if none.  A predicted record that is not matched
            has x_new = (float)iu, y_new = (float)iv, sad = second = INT32_MAX and PREDICTED alone.
  sub-pixel in x: iff the candidates (qx - 1, qy) and (qx + 1, qy) both lie in the search window and count,
            den = cm - 2 c0 + cp > 0 and c0 > 0:  x_new = (float)((double)qx + (double)(cm - cp) / (double)(2 den)), SUBPIX_X;
            otherwise x_new = (float)qx.  The same in y.  (c0 > 0: a perfect match stays on its pixel -- an unmoved or purely
            shifted image is tracked exactly, whatever its neighbours' SADs are.)
  fail      FAIL_SAD iff max_sad != 0 and sad > max_sad;  FAIL_GAP iff second != INT32_MAX and second - sad < min_gap.
  OK        flags & (PREDICTED | MATCHED | FAIL_SAD | FAIL_GAP) == PREDICTED | MATCHED.
  solve     see solve()'s own text: Gauss-Newton with Huber weights on the reprojection error, binary64.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

PREDICTED, MATCHED, SUBPIX_X, SUBPIX_Y, FAIL_SAD, FAIL_GAP = 1, 2, 4, 8, 16, 32
INT32_MAX = 2 ** 31 - 1
TRACK = np.dtype([("x", "<i4"), ("y", "<i4"), ("disp", "<f4"), ("x_new", "<f4"), ("y_new", "<f4"), ("sad", "<i4"),
                  ("second", "<i4"), ("flags", "<u4")])
assert TRACK.itemsize == 32
IDENTITY = (np.eye(3).ravel(), np.zeros(3))
TRACK_DEFAULTS = dict(cell=16, patch_radius=3, search_radius=5, min_score=1, min_disp=0.0, max_disp=0.0, max_sad=0, min_gap=0)
SOLVE_DEFAULTS = dict(iterations=10, huber_px=1.0, epsilon=1e-9, inlier_px=1.0, min_inliers=12)


# ---- tracking ----------------------------------------------------------------------------------------------------------------
def score(image):
    """-> int64 [rows][cols]; exact at every pixel at least 4 from the border, 0 in the border."""
    I = np.asarray(image, np.uint8).astype(np.int64)
    rows, cols = I.shape
    out = np.zeros((rows, cols), np.int64)
    if rows < 9 or cols < 9:
        return out
    gx = np.zeros((rows, cols), np.int64)
    gy = np.zeros((rows, cols), np.int64)
    a, b, c = I[:-2], I[1:-1], I[2:]
    gx[1:-1, 1:-1] = (a[:, 2:] + 2 * b[:, 2:] + c[:, 2:]) - (a[:, :-2] + 2 * b[:, :-2] + c[:, :-2])
    gy[1:-1, 1:-1] = (c[:, :-2] + 2 * c[:, 1:-1] + c[:, 2:]) - (a[:, :-2] + 2 * a[:, 1:-1] + a[:, 2:])
    box = lambda v: sliding_window_view(v, (7, 7)).sum(axis=(2, 3))
    sxx, syy, sxy = box(gx * gx), box(gy * gy), box(gx * gy)
    full = 16 * (sxx * syy - sxy * sxy) - (sxx + syy) ** 2
    out[4:-4, 4:-4] = full[1:-1, 1:-1]
    return out


def eligible(image, disp, patch_radius, min_score, min_disp, max_disp):
    """-> (bool [rows][cols], the score map)."""
    sc = score(image)
    d = np.asarray(disp, np.float32)
    rows, cols = d.shape
    m = max(int(patch_radius), 4)
    ok = np.zeros((rows, cols), bool)
    if rows >= 2 * m + 1 and cols >= 2 * m + 1:
        ok[m:rows - m, m:cols - m] = True
    with np.errstate(invalid="ignore"):
        ok &= np.isfinite(d) & (d > np.float32(0)) & (d >= np.float32(min_disp))
        if np.float32(max_disp) != np.float32(0):
            ok &= d <= np.float32(max_disp)
    ok &= sc >= np.int64(min_score)
    return ok, sc


def select(image, disp, cell, patch_radius, min_score, min_disp, max_disp):
    """-> the features' pixels (x, y) as an int64 [n][2] array, in record order."""
    ok, sc = eligible(image, disp, patch_radius, min_score, min_disp, max_disp)
    rows, cols = ok.shape
    found = []
    for y0 in range(0, rows, cell):
        for x0 in range(0, cols, cell):
            e = ok[y0:y0 + cell, x0:x0 + cell]
            if not e.any():
                continue
            s = sc[y0:y0 + cell, x0:x0 + cell]
            best = s[e].max()
            at = int(np.argmax((e & (s == best)).ravel()))  # the first in row-major order: the smallest y cols + x
            found.append((x0 + at % e.shape[1], y0 + at // e.shape[1]))
    return np.array(found, np.int64).reshape(-1, 2)


def point(camera, x, y, d):
    """pm_backproject's point before its rounding: binary64 (X, Y, Z) of pixel (x, y) with disparity d (arrays allowed)."""
    fx, fy, cx, cy, baseline = (np.float64(v) for v in camera)
    fxb = fx * baseline
    with np.errstate(all="ignore"):
        Z = fxb / np.asarray(d, np.float32).astype(np.float64)
        X = ((np.asarray(x, np.float64) - cx) * Z) / fx
        Y = ((np.asarray(y, np.float64) - cy) * Z) / fy
    return X, Y, Z


def transform(R, t, X, Y, Z):
    """R P + t in `splat`'s order."""
    R = np.asarray(R, np.float64).ravel()
    t = np.asarray(t, np.float64).ravel()
    with np.errstate(all="ignore"):
        Xn = (((R[0] * X) + (R[1] * Y)) + (R[2] * Z)) + t[0]
        Yn = (((R[3] * X) + (R[4] * Y)) + (R[5] * Z)) + t[1]
        Zn = (((R[6] * X) + (R[7] * Y)) + (R[8] * Z)) + t[2]
    return Xn, Yn, Zn


def predict(camera, R, t, x, y, d):
    """-> (predicted, iu, iv) of one pixel; iu, iv Python ints, 0 where not predicted."""
    fx, fy, cx, cy, _ = (np.float64(v) for v in camera)
    Xn, Yn, Zn = transform(R, t, *point(camera, x, y, d))
    with np.errstate(all="ignore"):
        u = (fx * (Xn / Zn)) + cx
        v = (fy * (Yn / Zn)) + cy
        ok = bool(Zn > 0) and bool(np.abs(u) < 2.0 ** 30) and bool(np.abs(v) < 2.0 ** 30)
    return (True, int(np.rint(u)), int(np.rint(v))) if ok else (False, 0, 0)


def sad_table(old, new, x, y, iu, iv, p, s):
    """-> int64 [(2s+1)][(2s+1)]: the SAD of every candidate, -1 where it does not count."""
    rows, cols = new.shape
    n1 = 2 * s + 1
    table = np.full((n1, n1), -1, np.int64)
    qx0, qx1 = max(iu - s, p), min(iu + s, cols - 1 - p)
    qy0, qy1 = max(iv - s, p), min(iv + s, rows - 1 - p)
    if qx0 > qx1 or qy0 > qy1:
        return table
    tmpl = old[y - p:y + p + 1, x - p:x + p + 1].astype(np.int64)
    region = new[qy0 - p:qy1 + p + 1, qx0 - p:qx1 + p + 1].astype(np.int64)
    win = sliding_window_view(region, (2 * p + 1, 2 * p + 1))
    table[qy0 - (iv - s):qy1 - (iv - s) + 1, qx0 - (iu - s):qx1 - (iu - s) + 1] = np.abs(win - tmpl).sum(axis=(2, 3))
    return table


def _subpix(q, cm, c0, cp):
    """-> (the binary32 position, whether the parabola was used); cm / cp: -1 where that neighbour does not count."""
    if cm >= 0 and cp >= 0 and c0 > 0:
        den = cm - 2 * c0 + cp
        if den > 0:
            return np.float32(np.float64(q) + np.float64(cm - cp) / np.float64(2 * den)), True
    return np.float32(q), False


def match(old, new, x, y, iu, iv, p, s, max_sad, min_gap):
    """One predicted record -> (x_new, y_new, sad, second, flags)."""
    table = sad_table(old, new, x, y, iu, iv, p, s)
    counts = table >= 0
    if not counts.any():
        return np.float32(iu), np.float32(iv), INT32_MAX, INT32_MAX, PREDICTED
    n1 = 2 * s + 1
    flat = np.where(counts, table, np.int64(1) << 40).ravel()
    at = int(np.argmin(flat))  # the first of the smallest
    by, bx = at // n1, at % n1
    sad = int(flat[at])
    yy, xx = np.mgrid[0:n1, 0:n1]
    far = counts & (np.maximum(np.abs(yy - by), np.abs(xx - bx)) >= 2)
    second = int(table[far].min()) if far.any() else INT32_MAX
    flags = PREDICTED | MATCHED
    tap = lambda j, i: int(table[j, i]) if 0 <= j < n1 and 0 <= i < n1 else -1
    x_new, used = _subpix(iu + bx - s, tap(by, bx - 1), sad, tap(by, bx + 1))
    flags |= SUBPIX_X if used else 0
    y_new, used = _subpix(iv + by - s, tap(by - 1, bx), sad, tap(by + 1, bx))
    flags |= SUBPIX_Y if used else 0
    if max_sad != 0 and sad > max_sad:
        flags |= FAIL_SAD
    if second != INT32_MAX and second - sad < min_gap:
        flags |= FAIL_GAP
    return x_new, y_new, sad, second, flags


def track(old, disp, new, camera, guess=None, cell=16, patch_radius=3, search_radius=5, min_score=1, min_disp=0.0,
          max_disp=0.0, max_sad=0, min_gap=0):
    """pm_track_features -> the records, a TRACK array (all of them: a capacity only truncates)."""
    old, new = np.asarray(old, np.uint8), np.asarray(new, np.uint8)
    disp = np.asarray(disp, np.float32)
    R, t = IDENTITY if guess is None else guess
    feats = select(old, disp, cell, patch_radius, min_score, min_disp, max_disp)
    out = np.zeros(len(feats), TRACK)
    for k, (x, y) in enumerate(feats):
        x, y = int(x), int(y)
        d = disp[y, x]
        ok, iu, iv = predict(camera, R, t, x, y, d)
        rec = (np.float32(0), np.float32(0), INT32_MAX, INT32_MAX, 0)
        if ok:
            rec = match(old, new, x, y, iu, iv, patch_radius, search_radius, max_sad, min_gap)
        out[k] = (x, y, d, *rec)
    return out


def ok_tracks(tracks):
    f = np.asarray(tracks)["flags"]
    return (f & (PREDICTED | MATCHED | FAIL_SAD | FAIL_GAP)) == (PREDICTED | MATCHED)


# ---- the solve ---------------------------------------------------------------------------------------------------------------
def _ordered_sum(terms):
    """From +0.0, in order, one rounding per addition (np.add.accumulate is sequential; np.sum is pairwise)."""
    return np.add.accumulate(np.concatenate([[np.float64(0.0)], np.asarray(terms, np.float64)]))[-1]


def residuals(camera, R, t, X, Y, Z, x_new, y_new):
    """-> (used, Qx, Qy, Qz, iz, a, b, ru, rv, e2, e) of every track under (R, t); `used`: Qz > 0."""
    fx, fy, cx, cy, _ = (np.float64(v) for v in camera)
    Qx, Qy, Qz = transform(R, t, X, Y, Z)
    with np.errstate(all="ignore"):
        used = Qz > 0
        iz = 1.0 / Qz
        a = Qx * iz
        b = Qy * iz
        ru = ((fx * a) + cx) - x_new
        rv = ((fy * b) + cy) - y_new
        e2 = (ru * ru) + (rv * rv)
        e = np.sqrt(e2)
    return used, Qx, Qy, Qz, iz, a, b, ru, rv, e2, e


def normal_equations(camera, R, t, X, Y, Z, x_new, y_new, huber_px):
    """-> (H: the 21 upper entries in row-major order (0,0), (0,1) .. (5,5); g[6]).  delta = (omega, upsilon) of the left
    perturbation Q' = Q + omega x Q + upsilon."""
    fx, fy, _, _, _ = (np.float64(v) for v in camera)
    used, Qx, Qy, Qz, iz, a, b, ru, rv, _, e = residuals(camera, R, t, X, Y, Z, x_new, y_new)
    pick = lambda v: v[used]
    Qx, Qy, Qz, iz, a, b, ru, rv, e = (pick(v) for v in (Qx, Qy, Qz, iz, a, b, ru, rv, e))
    with np.errstate(all="ignore"):
        w = np.where(e <= huber_px, np.float64(1.0), np.float64(huber_px) / e)
        A = fx * iz
        C = -((fx * a) * iz)
        B = fy * iz
        D = -((fy * b) * iz)
        zero = np.zeros_like(A)
        Ju = [C * Qy, (A * Qz) - (C * Qx), -(A * Qy), A, zero, C]
        Jv = [(D * Qy) - (B * Qz), -(D * Qx), B * Qx, zero, B, D]
        H = np.array([_ordered_sum(w * ((Ju[i] * Ju[j]) + (Jv[i] * Jv[j]))) for i in range(6) for j in range(i, 6)])
        g = np.array([_ordered_sum(w * ((Ju[i] * ru) + (Jv[i] * rv))) for i in range(6)])
    return H, g


def ldlt_solve(H21, g):
    """H delta = -g by LDL^T without pivoting, k ascending in every inner sum -> delta[6], or None where a pivot is not > 0."""
    H = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = H21[k]
            k += 1
    L, Dg = np.zeros((6, 6)), np.zeros(6)
    with np.errstate(all="ignore"):
        for j in range(6):
            s = H[j, j]
            for k in range(j):
                s = s - ((L[j, k] * L[j, k]) * Dg[k])
            if not s > 0:
                return None
            Dg[j] = s
            for i in range(j + 1, 6):
                s = H[j, i]
                for k in range(j):
                    s = s - ((L[i, k] * L[j, k]) * Dg[k])
                L[i, j] = s / Dg[j]
        yv = np.zeros(6)
        for i in range(6):
            s = -g[i]
            for k in range(i):
                s = s - (L[i, k] * yv[k])
            yv[i] = s
        z = yv / Dg
        delta = np.zeros(6)
        for i in range(5, -1, -1):
            s = z[i]
            for k in range(i + 1, 6):
                s = s - (L[k, i] * delta[k])
            delta[i] = s
    return delta


def cayley_update(R, t, delta):
    """a = omega / 2;  dR = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a);  R <- dR R;  t <- dR t + upsilon."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).ravel()
    with np.errstate(all="ignore"):
        a0, a1, a2 = (np.float64(0.5) * delta[i] for i in range(3))
        s = ((a0 * a0) + (a1 * a1)) + (a2 * a2)
        c, den = 1.0 - s, 1.0 + s
        dR = np.array([[(c + ((2 * a0) * a0)) / den, (((2 * a0) * a1) - (2 * a2)) / den, (((2 * a0) * a2) + (2 * a1)) / den],
                       [(((2 * a1) * a0) + (2 * a2)) / den, (c + ((2 * a1) * a1)) / den, (((2 * a1) * a2) - (2 * a0)) / den],
                       [(((2 * a2) * a0) - (2 * a1)) / den, (((2 * a2) * a1) + (2 * a0)) / den, (c + ((2 * a2) * a2)) / den]])
        Rn = np.array([[((dR[i, 0] * R[0, j]) + (dR[i, 1] * R[1, j])) + (dR[i, 2] * R[2, j]) for j in range(3)] for i in range(3)])
        tn = np.array([(((dR[i, 0] * t[0]) + (dR[i, 1] * t[1])) + (dR[i, 2] * t[2])) + delta[3 + i] for i in range(3)])
    return Rn.ravel(), tn


def solve(camera, tracks, guess=None, iterations=10, huber_px=1.0, epsilon=1e-9, inlier_px=1.0, min_inliers=12):
    """pm_solve_motion -> (R[9], t[3], info) with info = dict(valid, n_tracks, n_used, n_inliers, iterations, rms_px).
    Only OK tracks take part (n_tracks counts them); P_i is point() of (x, y, disp).  Per iteration the normal equations of the
    Huber-weighted reprojection error over the tracks with Qz > 0, in track order from +0.0; LDL^T; the Cayley update; it
    stops after the update when max |delta_i| < epsilon, or after `iterations` (info.iterations: the updates made).  A
    factorisation that fails ends the iterations.  Then under the motion reached: n_used (Qz > 0), the inliers (used and
    e <= inlier_px), rms_px = sqrt((sum of e^2 over the inliers, in order from +0.0) / n_inliers), 0 without an inlier.
    valid iff no factorisation failed and n_inliers >= min_inliers; where not valid, (R, t) is the guess."""
    R0, t0 = IDENTITY if guess is None else guess
    R0, t0 = np.asarray(R0, np.float64).ravel().copy(), np.asarray(t0, np.float64).ravel().copy()
    tr = np.asarray(tracks)
    tr = tr[ok_tracks(tr)]
    X, Y, Z = point(camera, tr["x"], tr["y"], tr["disp"])
    x_new, y_new = tr["x_new"].astype(np.float64), tr["y_new"].astype(np.float64)
    R, t, failed, done = R0, t0, False, 0
    for _ in range(iterations):
        H, g = normal_equations(camera, R, t, X, Y, Z, x_new, y_new, huber_px)
        delta = ldlt_solve(H, g)
        if delta is None:
            failed = True
            break
        R, t = cayley_update(R, t, delta)
        done += 1
        biggest = 0.0
        for v in np.abs(delta):
            biggest = float(v) if v > biggest else biggest  # a NaN is never the biggest
        if biggest < epsilon:
            break
    used, *_, e2, e = residuals(camera, R, t, X, Y, Z, x_new, y_new)
    with np.errstate(invalid="ignore"):
        inl = used & (e <= inlier_px)
    n_in = int(inl.sum())
    rms = np.sqrt(_ordered_sum(e2[inl]) / np.float64(n_in)) if n_in else np.float64(0.0)
    valid = (not failed) and n_in >= min_inliers
    info = dict(valid=int(valid), n_tracks=len(tr), n_used=int(used.sum()), n_inliers=n_in, iterations=done, rms_px=float(rms))
    return (R, t, info) if valid else (R0, t0, info)


def estimate(old, disp, new, camera, guess=None, track_options=None, solve_options=None):
    """pm_estimate_motion -> (R, t, info, tracks)."""
    tracks = track(old, disp, new, camera, guess, **dict(TRACK_DEFAULTS, **(track_options or {})))
    R, t, info = solve(camera, tracks, guess, **dict(SOLVE_DEFAULTS, **(solve_options or {})))
    return R, t, info, tracks
