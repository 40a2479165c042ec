"""The definition of pm_fuse_disparity (include/pm/imaging.h) in numpy: the CURRENT left disparity map refined by, and filled
from, n earlier left maps of the same size and rectified camera, each reached through the rigid motion between the two left
cameras (X_src_k = R X_cur + t, pm_filter_consistency's convention).  The kernels are held to it with tolerance 0, like
tests/consistency_ref.py: every operation below is ONE rounding in the format named, with the parentheses as written.

  refine    a pixel is valid iff d = D(y, x) > 0 (binary32).  project, tap and class are consistency_ref's, unchanged
            (max_diff, radius); Z = fxB / (double)d and Zn are the values `project` formed.  A CONSISTENT source k with the
            chosen tap's ds gives, in binary64:  Zs = fxB / (double)ds;  g = Zn - t2;  Zo = ((Zs - t2) * Z) / g;
            o_k = fxB / Zo.  It takes part iff g > 0, Zo > 0, o_k is finite and its weight w_k > 0.  Weights: w0 =
            W(y, x), w_k = W_k at the chosen tap, 1.0 for a plane that is not given; (double)w iff w is finite and > 0, else 0.
            num = w0 * (double)d, den = w0; then for k = 0 .. n - 1 in order, the sources that take part:
            num = num + (w_k * o_k), den = den + w_k.  omin / omax: over (double)d where w0 > 0 and the o_k that take part.
            KEPT iff valid, n_cons >= min_consistent and n_conf <= max_conflicts.
            out: not KEPT +0.0f; KEPT and den > 0 (float)(num / den); KEPT otherwise the input bits.  A NaN quotient (a
            valid pixel that is +inf with w0 = 0) is the canonical quiet NaN 0x7FC00000.
            count: the observations that took part (the pixel's own included where w0 > 0), 0 .. 9.
            spread: (float)(omax - omin), +0.0 where count == 0; a NaN (+inf - +inf, a valid pixel that is +inf) is the
            canonical quiet NaN 0x7FC00000.
  fill      only with fill_min_sources >= 1.  Rinv[3i+j] = R[3j+i];  tinv_i = -(((R[i]*t0) + (R[3+i]*t1)) + (R[6+i]*t2)).
            S_k = reproject_ref.splat_left(source k, camera, Rinv, tinv) (min_disp = max_disp = 0, no close).  At an invalid
            pixel: c_k = S_k(y, x), a candidate iff c_k > 0; m = their binary32 maximum; k SUPPORTS iff c_k > 0 and
            fabs((double)c_k - (double)m) <= (double)fill_max_diff; FILLED iff n_sup >= fill_min_sources (and n_sup >= 1);
            acc from +0.0 in k order over the supporters, acc = acc + (double)c_k; out = (float)(acc / (double)n_sup);
            count = n_sup; spread = (float)((double)m - (double)(the smallest supporter)).  Not filled: the input bits,
            count 0, spread +0.0.
  flags     VALID 1, KEPT 2, FUSED 4 (kept and at least one SOURCE observation took part), FILLED 8.
  counts    int32 [valid, kept, fused, filled].
"""
import numpy as np

import consistency_ref as CR
import reproject_ref as RR

VALID, KEPT, FUSED, FILLED = 1, 2, 4, 8
MAX_SOURCES = CR.MAX_SOURCES


def inverse_motion(R, t):
    """(Rinv[9], tinv[3]) in binary64, the parentheses of the definition."""
    R = np.asarray(R, np.float64).ravel()
    t = np.asarray(t, np.float64).ravel()
    Rinv = np.array([R[3 * j + i] for i in range(3) for j in range(3)], np.float64)
    tinv = np.array([-(((R[i] * t[0]) + (R[3 + i] * t[1])) + (R[6 + i] * t[2])) for i in range(3)], np.float64)
    return Rinv, tinv


def weight64(w):
    """(double)w where w is finite and > 0, else 0."""
    w = np.asarray(w, np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(w) & (w > np.float32(0))
    return np.where(ok, w, np.float32(0)).astype(np.float64)


def depths(disp, camera, R, t):
    """Z and Zn of consistency_ref.project, which keeps them to itself: the same operations in the same order."""
    fx, fy, cx, cy, baseline = (np.float64(v) for v in camera)
    R = np.asarray(R, np.float64).ravel()
    t = np.asarray(t, np.float64).ravel()
    disp = np.asarray(disp, np.float32)
    rows, cols = disp.shape
    fxb = fx * baseline
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        ok = disp > np.float32(0)
        Z = fxb / np.where(ok, disp, np.float32(1)).astype(np.float64)
        X = ((x - cx) * Z) / fx
        Y = ((y - cy) * Z) / fy
        Zn = (((R[6] * X) + (R[7] * Y)) + (R[8] * Z)) + t[2]
    return Z, Zn


def chosen_tap(disp, source, camera, R, t, max_diff, radius):
    """consistency_ref.classify, which also says WHICH tap it chose -> (class uint8, ds float32, ty, tx int64; ds = 0 and
    (0, 0) where UNSEEN)."""
    source = np.asarray(source, np.float32)
    rows, cols = source.shape
    seen, iu, iv, dp = CR.project(disp, camera, R, t)
    dp64 = dp.astype(np.float64)
    found = np.zeros((rows, cols), bool)
    best = np.zeros((rows, cols), np.float64)
    e = np.zeros((rows, cols), np.float64)
    sel = np.zeros((rows, cols), np.float32)
    ty = np.zeros((rows, cols), np.int64)
    tx = np.zeros((rows, cols), np.int64)
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
                sel = np.where(take, ds, sel)
                ty = np.where(take, yy, ty)
                tx = np.where(take, xx, tx)
                found |= take
        md = np.float64(np.float32(max_diff))
        cls = np.where(best <= md, CR.CONSISTENT, np.where(e > md, CR.OCCLUDED, CR.CONFLICT))
    cls = np.where(found, cls, CR.UNSEEN).astype(np.uint8)
    return cls, sel.astype(np.float32), ty, tx


def _canonical(a):
    """A NaN becomes the canonical quiet NaN 0x7FC00000: the sign of a generated NaN differs between processors."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32)).astype(np.uint32).view(np.float32)


def fill_splats(sources, camera, motions):
    """[n][rows][cols] float32: source k carried into the current view through the inverse of motions[k]."""
    return np.stack([RR.splat_left(s, camera, *inverse_motion(*m))[0] for s, m in zip(sources, motions)])


def fuse(disp, sources, camera, motions, weight=None, source_weights=None, max_diff=1.0, radius=1, min_consistent=1,
         max_conflicts=0, fill_min_sources=0, fill_max_diff=1.0):
    """-> dict(out float32, count uint8, spread float32, flags uint8 [rows][cols]; counts int32[4]; per_source uint8
    [n][rows][cols]; splats float32 [n][rows][cols] or None)."""
    disp = np.asarray(disp, np.float32)
    n = len(sources)
    assert 1 <= n <= MAX_SOURCES and len(motions) == n and 0 <= fill_min_sources <= n
    rows, cols = disp.shape
    fx, fy, cx, cy, baseline = (np.float64(v) for v in camera)
    fxb = fx * baseline
    if source_weights is None:
        source_weights = [None] * n
    with np.errstate(invalid="ignore"):
        valid = disp > np.float32(0)
    w0 = weight64(weight) if weight is not None else np.ones((rows, cols), np.float64)
    d64 = disp.astype(np.float64)
    own = valid & (w0 > 0)
    with np.errstate(invalid="ignore", over="ignore"):
        num = w0 * d64
    den = w0.copy()
    omin = np.where(own, d64, np.inf)
    omax = np.where(own, d64, -np.inf)
    count = own.astype(np.int32)
    n_src = np.zeros((rows, cols), np.int32)
    n_cons = np.zeros((rows, cols), np.int32)
    n_conf = np.zeros((rows, cols), np.int32)
    per_source = np.zeros((n, rows, cols), np.uint8)
    for k in range(n):
        R, t = motions[k]
        t2 = np.float64(np.asarray(t, np.float64).ravel()[2])
        cls, ds, ty, tx = chosen_tap(disp, sources[k], camera, R, t, max_diff, radius)
        per_source[k] = cls
        cons = valid & (cls == CR.CONSISTENT)
        n_cons += cons
        n_conf += valid & (cls == CR.CONFLICT)
        Z, Zn = depths(disp, camera, R, t)
        wk = weight64(np.asarray(source_weights[k], np.float32)[ty, tx]) if source_weights[k] is not None else np.ones((rows, cols))
        with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
            Zs = fxb / np.where(cons, ds, np.float32(1)).astype(np.float64)
            g = Zn - t2
            Zo = ((Zs - t2) * Z) / g
            o = fxb / Zo
            part = cons & (g > 0) & (Zo > 0) & np.isfinite(o) & (wk > 0)
            num = np.where(part, num + (wk * o), num)
            den = np.where(part, den + wk, den)
        omin = np.where(part & (o < omin), o, omin)
        omax = np.where(part & (o > omax), o, omax)
        count += part
        n_src += part
    kept = valid & (n_cons >= min_consistent) & (n_conf <= max_conflicts)
    fused = kept & (n_src > 0)
    out = disp.copy()
    out[valid & ~kept] = np.float32(0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        mean = (num / den).astype(np.float32)
        sp = (omax - omin).astype(np.float32)
    take = kept & (den > 0)
    out[take] = mean[take]
    mean, sp = _canonical(mean), _canonical(sp)
    spread = np.where(valid & (count > 0), sp, np.float32(0)).astype(np.float32)
    count = np.where(valid, count, 0)
    filled = np.zeros((rows, cols), bool)
    splats = None
    if fill_min_sources >= 1:
        splats = fill_splats(sources, camera, motions)
        cand = splats > np.float32(0)
        m = np.where(cand, splats, np.float32(0)).max(axis=0)
        fmd = np.float64(np.float32(fill_max_diff))
        sup = cand & (np.abs(splats.astype(np.float64) - m.astype(np.float64)[None]) <= fmd)
        n_sup = sup.sum(axis=0).astype(np.int32)
        filled = ~valid & (n_sup >= max(fill_min_sources, 1))
        acc = np.zeros((rows, cols), np.float64)
        for k in range(n):
            acc = np.where(sup[k], acc + splats[k].astype(np.float64), acc)
        lo = np.where(sup, splats, np.float32(np.inf)).min(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            val = (acc / np.maximum(n_sup, 1).astype(np.float64)).astype(np.float32)
            fsp = (m.astype(np.float64) - np.where(n_sup > 0, lo, np.float32(0)).astype(np.float64)).astype(np.float32)
        out[filled] = val[filled]
        count = np.where(filled, n_sup, count)
        spread = np.where(filled, fsp, spread).astype(np.float32)
    flags = (valid * VALID + kept * KEPT + fused * FUSED + filled * FILLED).astype(np.uint8)
    counts = np.array([valid.sum(), kept.sum(), fused.sum(), filled.sum()], np.int32)
    return dict(out=out, count=count.astype(np.uint8), spread=spread, flags=flags, counts=counts, per_source=per_source,
                splats=splats, valid=valid, kept=kept, fused=fused, filled=filled)
