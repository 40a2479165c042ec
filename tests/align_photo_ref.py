"""The definition of pm_bgr_luma, pm_align_photo_evaluate, pm_align_sums_blend and pm_align_color_disparity
(include/pm/imaging.h) in numpy: a PHOTOMETRIC term for the dense alignment of tests/align_ref.py.  A model pixel's luma
(pm_tsdf_color_map's colour of the model, through pm_bgr_luma) is compared with the new image's luma at the place the pixel
projects to, sampled bilinearly; the normal equations it gives have align_ref's shape and are blended into align_ref's.
The kernels are held to it with tolerance 0: every operation below is ONE rounding in binary64 unless binary32 is named, with the
parentheses as written.  The motion, the camera, the classes, the 28 terms and the ORDER of the sum are align_ref's, reused.

luma, per pixel, binary32: p_c = (float)byte or the float as it is; L = ((b * 0.114f) + (g * 0.587f)) + (r * 0.299f).  The output
is the quiet NaN 0x7FC00000 where a channel is not finite, or where zero_is_absent and all three channels == 0 (how
pm_tsdf_color_map marks "not coloured").  NaN is the one "absent" marker of a luma plane.

Per model pixel (x, y):
  model     d = Dm(y, x) counts iff d > 0 and d >= min_disp (binary32); Lm = (double)Lum_m(y, x) counts iff finite.  Otherwise
            NO_MODEL.  P = align_ref.point.
  project   align_ref.project: Q = (Xn, Yn, Zn), dq, (iu, iv); a dropped pixel is OUTSIDE.  u = (fx * (Xn / Zn)) + cx;
            v = (fy * (Yn / Zn)) + cy (project's own expressions); x0 = floor(u); y0 = floor(v); OUTSIDE also unless
            x0 >= 0 and x0 + 1 <= cols - 1 and y0 >= 0 and y0 + 1 <= rows - 1.
  measure   d2 = Dn(iv, iu) counts as d does; L00 = Ln(y0, x0), L01 = Ln(y0, x0 + 1), L10 = Ln(y0 + 1, x0),
            L11 = Ln(y0 + 1, x0 + 1) are all finite.  Otherwise UNMEASURED.
  gate      fabs((double)dq - (double)d2) <= (double)max_diff; otherwise GATED.
  sample    the taps converted to binary64; a = u - (double)x0; b = v - (double)y0; dt = L01 - L00; db = L11 - L10;
            top = L00 + (a * dt); bot = L10 + (a * db); val = top + (b * (bot - top)); gx = dt + (b * (db - dt)); gy = bot - top.
  residual  r = val - Lm, in levels.
  row       bx = (gx * fx) / Qz; by = (gy * fy) / Qz; bz = -(((bx * Qx) + (by * Qy)) / Qz);
            J = ((Qy*bz) - (Qz*by), (Qz*bx) - (Qx*bz), (Qx*by) - (Qy*bx), bx, by, bz).
  weight    ar = fabs(r); w = 1.0 if ar <= huber_levels, else huber_levels / ar.
  terms     align_ref's 28 and its ordered_sum.  USED; any other class adds +0.0 to all 28.
blend: l2 = lambda * lambda; each of the 28 doubles is geo + (l2 * photo); the three counts are integer sums.
The loop (align_color) is align_ref.align's with the blended record in front of every step."""
import numpy as np

import align_ref as AR

NO_MODEL, OUTSIDE, UNMEASURED, GATED, USED = range(5)
ABSENT = np.uint32(0x7FC00000).view(np.float32)
PHOTO_OPTIONS = dict(min_disp=0.0, max_diff=1.0, huber_levels=20.0)
COLOR_OPTIONS = dict(AR.OPTIONS, huber_levels=20.0, lam=0.03)


def photo_options(**kw):
    o = dict(PHOTO_OPTIONS)
    o.update(kw)
    return o


def color_options(**kw):
    """pm_align_color_options: align_ref.OPTIONS' fields (the geometric term and the loop), huber_levels and lam (lambda)."""
    o = dict(COLOR_OPTIONS)
    o.update(kw)
    return o


def luma(image, zero_is_absent):
    """pm_bgr_luma: image uint8 or float32 [rows][cols][3] -> float32 [rows][cols]."""
    image = np.asarray(image)
    assert image.dtype in (np.uint8, np.float32) and image.shape[-1] == 3
    p = image.astype(np.float32)
    with np.errstate(all="ignore"):
        L = ((p[..., 0] * np.float32(0.114)) + (p[..., 1] * np.float32(0.587))) + (p[..., 2] * np.float32(0.299))
    absent = ~np.isfinite(p).all(-1)
    if zero_is_absent:
        absent |= (p == 0).all(-1)
    return np.where(absent, ABSENT, L).astype(np.float32)


def pixel_terms(camera, opt, motion, disp_model, luma_model, disp_new, luma_new):
    """-> (cls uint8 [rows][cols], r float64 [rows][cols] (0 unless USED), terms float64 [rows][cols][28] (+0.0 unless USED),
    gradient float64 [rows][cols][2] (gx, gy; 0 unless USED))."""
    Dm = np.ascontiguousarray(disp_model, np.float32)
    Lm32 = np.ascontiguousarray(luma_model, np.float32)
    Dn = np.ascontiguousarray(disp_new, np.float32)
    Ln = np.ascontiguousarray(luma_new, np.float32)
    rows, cols = Dm.shape
    assert Lm32.shape == (rows, cols) and Dn.shape == (rows, cols) and Ln.shape == (rows, cols)
    R = np.asarray(motion[0], np.float64).ravel()
    t = np.asarray(motion[1], np.float64).ravel()
    fx, fy, cx, cy = (np.float64(v) for v in camera[:4])
    x = np.broadcast_to(np.arange(cols)[None, :], (rows, cols))
    y = np.broadcast_to(np.arange(rows)[:, None], (rows, cols))
    with np.errstate(all="ignore"):
        has_d, X, Y, Z = AR.point(camera, Dm, x, y, opt["min_disp"])
        model = has_d & np.isfinite(Lm32)
        Lm = Lm32.astype(np.float64)
        kept, iu, iv, dq, Qx, Qy, Qz = AR.project(camera, R, t, X, Y, Z, rows, cols)
        kept &= model
        u = np.where(kept, (fx * (Qx / Qz)) + cx, 0.0)
        v = np.where(kept, (fy * (Qy / Qz)) + cy, 0.0)
        x0f, y0f = np.floor(u), np.floor(v)
        kept &= (x0f >= 0) & (x0f + 1 <= cols - 1) & (y0f >= 0) & (y0f + 1 <= rows - 1)
        x0 = np.where(kept, x0f, 0).astype(np.int64)
        y0 = np.where(kept, y0f, 0).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, cols - 1), np.minimum(y0 + 1, rows - 1)  # (equal to x0 + 1, y0 + 1 wherever kept)
        d2 = Dn[np.where(kept, iv, 0), np.where(kept, iu, 0)]
        measured = (d2 > np.float32(0)) & (d2 >= np.float32(opt["min_disp"]))
        L00, L01, L10, L11 = Ln[y0, x0], Ln[y0, x1], Ln[y1, x0], Ln[y1, x1]
        measured &= np.isfinite(L00) & np.isfinite(L01) & np.isfinite(L10) & np.isfinite(L11)
        measured &= kept
        gate = np.abs(dq.astype(np.float64) - d2.astype(np.float64)) <= np.float64(np.float32(opt["max_diff"]))
        used = measured & gate
        cls = np.where(~model, NO_MODEL, np.where(~kept, OUTSIDE, np.where(~measured, UNMEASURED, np.where(~gate, GATED, USED))))
        L00, L01, L10, L11 = (a.astype(np.float64) for a in (L00, L01, L10, L11))
        a = u - x0f
        b = v - y0f
        dt = L01 - L00
        db = L11 - L10
        top = L00 + (a * dt)
        bot = L10 + (a * db)
        val = top + (b * (bot - top))
        gx = dt + (b * (db - dt))
        gy = bot - top
        r = val - Lm
        bx = (gx * fx) / Qz
        by = (gy * fy) / Qz
        bz = -(((bx * Qx) + (by * Qy)) / Qz)
        J = [(Qy * bz) - (Qz * by), (Qz * bx) - (Qx * bz), (Qx * by) - (Qy * bx), bx, by, bz]
        ar = np.abs(r)
        huber = np.float64(opt["huber_levels"])
        w = np.where(ar <= huber, np.float64(1.0), huber / ar)
        terms = [(w * J[j]) * J[k] for j in range(6) for k in range(j, 6)] + [(w * J[j]) * r for j in range(6)] + [r * r]
        terms = np.stack([np.where(used, q, np.float64(0.0)) for q in terms], -1)
        grad = np.stack([np.where(used, gx, 0.0), np.where(used, gy, 0.0)], -1)
    return cls.astype(np.uint8), np.where(used, r, np.float64(0.0)), terms, grad


def evaluate(camera, opt, motion, disp_model, luma_model, disp_new, luma_new):
    """pm_align_photo_evaluate -> align_ref.evaluate's dict, and `gradient` [rows][cols][2]."""
    cls, r, terms, grad = pixel_terms(camera, opt, motion if motion is not None else AR.IDENTITY, disp_model, luma_model, disp_new,
                                      luma_new)
    total, row_sums = AR.ordered_sum(terms)
    return dict(cls=cls, residual=r.astype(np.float32), H=total[:21].copy(), g=total[21:27].copy(), rr=total[27],
                n_model=int((cls != NO_MODEL).sum()), n_gate=int((cls >= GATED).sum()), n_used=int((cls == USED).sum()),
                row_sums=row_sums, gradient=grad)


def blend(geo, photo, lam):
    """pm_align_sums_blend on two evaluations' dicts -> dict(H, g, rr, n_model, n_gate, n_used)."""
    with np.errstate(all="ignore"):
        l2 = np.float64(lam) * np.float64(lam)
        out = {k: np.asarray(geo[k], np.float64) + (l2 * np.asarray(photo[k], np.float64)) for k in ("H", "g", "rr")}
    out["rr"] = np.float64(out["rr"])
    for k in ("n_model", "n_gate", "n_used"):
        out[k] = int(geo[k]) + int(photo[k])
    return out


def align_color(camera, opt, guess, disp_model, normals_model, bgr_model, disp_new, image_new):
    """pm_align_color_disparity -> ((R[9], t[3]), info): info = dict(geo = align_ref.align's info, n_photo_model, n_photo_gate,
    n_photo_used, rms_levels, H[21] the blended matrix).  bgr_model float32 [rows][cols][3]; image_new uint8 or float32."""
    geo_opt = {k: opt[k] for k in AR.OPTIONS}
    pho_opt = dict(min_disp=opt["min_disp"], max_diff=opt["max_diff"], huber_levels=opt["huber_levels"])
    lm = luma(np.asarray(bgr_model, np.float32), True)
    ln = luma(image_new, False)
    start = (np.asarray((guess or AR.IDENTITY)[0], np.float64).ravel().copy(), np.asarray((guess or AR.IDENTITY)[1], np.float64).ravel().copy())

    def both(m):
        g = AR.evaluate(camera, geo_opt, m, disp_model, normals_model, disp_new)
        p = evaluate(camera, pho_opt, m, disp_model, lm, disp_new, ln)
        return g, p, blend(g, p, opt["lam"])

    m, failed, done = start, False, 0
    for _ in range(opt["iterations"]):
        _, _, s = both(m)
        ok, m2, delta = AR.step(s["H"], s["g"], m)
        if not ok:
            failed = True
            break
        m = m2
        done += 1
        biggest = 0.0
        for q in delta:
            biggest = abs(q) if abs(q) > biggest else biggest
        if biggest < opt["epsilon"]:
            break
    g, p, s = both(m)
    valid = (not failed) and g["n_used"] + p["n_used"] >= opt["min_used"]
    with np.errstate(all="ignore"):
        rms = float(np.sqrt(g["rr"] / np.float64(g["n_used"]))) if g["n_used"] else 0.0
        rms_levels = float(np.sqrt(p["rr"] / np.float64(p["n_used"]))) if p["n_used"] else 0.0
    geo = dict(valid=int(valid), n_model=g["n_model"], n_gate=g["n_gate"], n_used=g["n_used"], iterations=done, rms_px=rms, H=g["H"])
    info = dict(geo=geo, n_photo_model=p["n_model"], n_photo_gate=p["n_gate"], n_photo_used=p["n_used"], rms_levels=rms_levels,
                H=s["H"])
    return (m if valid else start), info
