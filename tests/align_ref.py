"""The definition of pm_align_evaluate, pm_align_step, pm_align_disparity and pm_motion_compose (include/pm/imaging.h) in numpy:
dense point-to-plane alignment of a NEW disparity map against a MODEL's disparity map and normals, with projective association.
The kernels are held to it with tolerance 0, like tests/tsdf_ref.py: every operation below is ONE rounding in binary64 unless
binary32 is named, with the parentheses as written (numpy's element-wise +, -, *, /, rint and abs are IEEE operations).

The motion (R[9], t[3]) goes from the MODEL camera frame into the NEW camera frame, X_new = R X_model + t
(pm_reproject_disparity's convention).  camera: (fx, fy, cx, cy, baseline); fxB = fx * baseline.

Per model pixel (x, y):
  model     d = Dm(y, x) counts iff d > 0 and d >= min_disp (binary32); n = Nm(y, x, :) counts iff finite and not all zero;
            Z = fxB / (double)d; P = ((((double)x - cx) * Z) / fx, (((double)y - cy) * Z) / fy, Z).  Otherwise NO_MODEL.
  project   reproject_ref.splat_left's lines with max_disp = 0: Q = (Xn, Yn, Zn); dropped unless Zn > 0; dq = (float)(fxB / Zn)
            must be > 0 and finite; u = (fx * (Xn / Zn)) + cx, v likewise; |u|, |v| < 2^30; (iu, iv) = rint; inside the image.
            A dropped pixel is OUTSIDE.
  measure   d2 = Dn(iv, iu) counts iff d2 > 0 and d2 >= min_disp; otherwise UNMEASURED.
  gate      fabs((double)dq - (double)d2) <= (double)max_diff; otherwise GATED.
  point     P2 = the point of (d2, iu, iv), as P.
  normal    m_i = ((R[3i]*(double)n0) + (R[3i+1]*(double)n1)) + (R[3i+2]*(double)n2).
  residual  e = ((m0*(Qx-P2x)) + (m1*(Qy-P2y))) + (m2*(Qz-P2z));  s = (P2z*P2z) / fxB;  r = e / s.
  row       a0 = (P2y*m2) - (P2z*m1); a1 = (P2z*m0) - (P2x*m2); a2 = (P2x*m1) - (P2y*m0); J = (a0, a1, a2, m0, m1, m2), each / s.
  weight    ar = fabs(r); w = 1.0 if ar <= huber_px, else huber_px / ar.
  terms     H_jk = (w*J_j)*J_k, j <= k, row-major (21); g_j = (w*J_j)*r (6); r*r (1).  USED; any other class adds +0.0 to all 28.
The sum (ordered_sum): lane sums A[y][l] over c ascending from +0.0 of term(y, 64c + l), +0.0 beyond cols; the balanced tree
s[i] = s[2i] + s[2i+1] six times over l; the rows in ascending y from +0.0.
The solve (step) is tests/motion_ref.py's ldlt_solve and cayley_update; the loop (align) is pm_solve_motion's."""
import numpy as np

import motion_ref as MR

NO_MODEL, OUTSIDE, UNMEASURED, GATED, USED = range(5)
LANES, TERMS = 64, 28
IDENTITY = (np.eye(3).ravel(), np.zeros(3))
OPTIONS = dict(min_disp=0.0, max_diff=1.0, huber_px=1.0, iterations=10, epsilon=1e-9, min_used=100)


def options(**kw):
    o = dict(OPTIONS)
    o.update(kw)
    return o


def point(camera, d, x, y, min_disp):
    """reproject_point: (counts, X, Y, Z); d float32, x, y integer arrays."""
    fx, fy, cx, cy, baseline = (np.float64(v) for v in camera)
    fxb = fx * baseline
    with np.errstate(all="ignore"):
        ok = (d > np.float32(0)) & (d >= np.float32(min_disp))
        Z = fxb / np.where(ok, d, np.float32(1)).astype(np.float64)
        X = ((x.astype(np.float64) - cx) * Z) / fx
        Y = ((y.astype(np.float64) - cy) * Z) / fy
    return ok, X, Y, Z


def project(camera, R, t, X, Y, Z, rows, cols):
    """reproject_project with max_disp = 0 -> (kept, iu, iv (0 where dropped), dq float32, Xn, Yn, Zn)."""
    fx, fy, cx, cy, baseline = (np.float64(v) for v in camera)
    fxb = fx * baseline
    with np.errstate(all="ignore"):
        Xn = (((R[0] * X) + (R[1] * Y)) + (R[2] * Z)) + t[0]
        Yn = (((R[3] * X) + (R[4] * Y)) + (R[5] * Z)) + t[1]
        Zn = (((R[6] * X) + (R[7] * Y)) + (R[8] * Z)) + t[2]
        ok = Zn > 0
        dq = (fxb / Zn).astype(np.float32)
        ok &= (dq > np.float32(0)) & np.isfinite(dq)
        u = (fx * (Xn / Zn)) + cx
        v = (fy * (Yn / Zn)) + cy
        ok &= (np.abs(u) < 2.0 ** 30) & (np.abs(v) < 2.0 ** 30)
        iu, iv = np.rint(u), np.rint(v)
        ok &= (iu >= 0) & (iu < cols) & (iv >= 0) & (iv < rows)
    iu = np.where(ok, iu, 0).astype(np.int64)
    iv = np.where(ok, iv, 0).astype(np.int64)
    return ok, iu, iv, dq, Xn, Yn, Zn


def pixel_terms(camera, opt, motion, disp_model, normals_model, disp_new):
    """-> (cls uint8 [rows][cols], r float64 [rows][cols] (0 unless USED), terms float64 [rows][cols][28] (+0.0 unless USED))."""
    Dm = np.ascontiguousarray(disp_model, np.float32)
    Nm = np.ascontiguousarray(normals_model, np.float32)
    Dn = np.ascontiguousarray(disp_new, np.float32)
    rows, cols = Dm.shape
    assert Nm.shape == (rows, cols, 3) and Dn.shape == (rows, cols)
    R = np.asarray(motion[0], np.float64).ravel()
    t = np.asarray(motion[1], np.float64).ravel()
    fxb = np.float64(camera[0]) * np.float64(camera[4])
    x = np.broadcast_to(np.arange(cols)[None, :], (rows, cols))
    y = np.broadcast_to(np.arange(rows)[:, None], (rows, cols))
    with np.errstate(all="ignore"):
        has_d, X, Y, Z = point(camera, Dm, x, y, opt["min_disp"])
        has_n = np.isfinite(Nm).all(-1) & ~(Nm == 0).all(-1)
        model = has_d & has_n
        kept, iu, iv, dq, Qx, Qy, Qz = project(camera, R, t, X, Y, Z, rows, cols)
        kept &= model
        d2 = Dn[np.where(kept, iv, 0), np.where(kept, iu, 0)]
        measured, P2x, P2y, P2z = point(camera, d2, np.where(kept, iu, 0), np.where(kept, iv, 0), opt["min_disp"])
        measured &= kept
        gate = np.abs(dq.astype(np.float64) - d2.astype(np.float64)) <= np.float64(np.float32(opt["max_diff"]))
        used = measured & gate
        cls = np.where(~model, NO_MODEL, np.where(~kept, OUTSIDE, np.where(~measured, UNMEASURED, np.where(~gate, GATED, USED))))
        n0, n1, n2 = (Nm[..., i].astype(np.float64) for i in range(3))
        m0 = ((R[0] * n0) + (R[1] * n1)) + (R[2] * n2)
        m1 = ((R[3] * n0) + (R[4] * n1)) + (R[5] * n2)
        m2 = ((R[6] * n0) + (R[7] * n1)) + (R[8] * n2)
        e = ((m0 * (Qx - P2x)) + (m1 * (Qy - P2y))) + (m2 * (Qz - P2z))
        s = (P2z * P2z) / fxb
        r = e / s
        J = [((P2y * m2) - (P2z * m1)) / s, ((P2z * m0) - (P2x * m2)) / s, ((P2x * m1) - (P2y * m0)) / s, m0 / s, m1 / s, m2 / s]
        ar = np.abs(r)
        huber = np.float64(opt["huber_px"])
        w = np.where(ar <= huber, np.float64(1.0), huber / ar)
        terms = [(w * J[j]) * J[k] for j in range(6) for k in range(j, 6)] + [(w * J[j]) * r for j in range(6)] + [r * r]
        terms = np.stack([np.where(used, v, np.float64(0.0)) for v in terms], -1)
    return cls.astype(np.uint8), np.where(used, r, np.float64(0.0)), terms


def tree(A):
    """The balanced binary tree over the last axis (64 values): s[i] = s[2i] + s[2i+1], six times."""
    assert A.shape[-1] == LANES
    with np.errstate(all="ignore"):
        while A.shape[-1] > 1:
            A = A[..., 0::2] + A[..., 1::2]
    return A[..., 0]


def ordered_sum(terms):
    """terms [rows][cols][28] -> (total [28], row sums [rows][28]) in the definition's order."""
    rows, cols, n = terms.shape
    chunks = (cols + LANES - 1) // LANES
    padded = np.zeros((rows, chunks * LANES, n))
    padded[:, :cols] = terms
    padded = padded.reshape(rows, chunks, LANES, n)
    with np.errstate(all="ignore"):
        A = np.zeros((rows, LANES, n))
        for c in range(chunks):
            A = A + padded[:, c]
        row_sums = tree(np.moveaxis(A, 1, -1))  # [rows][28]
        total = np.zeros(n)
        for y in range(rows):
            total = total + row_sums[y]
    return total, row_sums


def evaluate(camera, opt, motion, disp_model, normals_model, disp_new):
    """pm_align_evaluate -> dict(cls uint8, residual float32, H[21], g[6], rr, n_model, n_gate, n_used, row_sums)."""
    cls, r, terms = pixel_terms(camera, opt, motion if motion is not None else IDENTITY, disp_model, normals_model, disp_new)
    total, row_sums = ordered_sum(terms)
    return dict(cls=cls, residual=r.astype(np.float32), H=total[:21].copy(), g=total[21:27].copy(), rr=total[27],
                n_model=int((cls != NO_MODEL).sum()), n_gate=int((cls >= GATED).sum()), n_used=int((cls == USED).sum()),
                row_sums=row_sums)


def record(ev):
    """The 240 bytes of pm_align_sums."""
    return np.concatenate([np.concatenate([ev["H"], ev["g"], [ev["rr"]]]).astype(np.float64).view(np.uint8),
                           np.array([ev["n_model"], ev["n_gate"], ev["n_used"], 0], np.int32).view(np.uint8)])


def step(H21, g, motion):
    """pm_align_step -> (factorised, (R[9], t[3]), delta[6]); the motion unchanged and delta +0.0 where the factorisation fails."""
    R = np.asarray(motion[0], np.float64).ravel().copy()
    t = np.asarray(motion[1], np.float64).ravel().copy()
    delta = MR.ldlt_solve(np.asarray(H21, np.float64), np.asarray(g, np.float64))
    if delta is None:
        return False, (R, t), np.zeros(6)
    Rn, tn = MR.cayley_update(R, t, delta)
    return True, (Rn, tn), delta


def compose(a, b):
    """pm_motion_compose: X -> a(b(X))."""
    aR, at = np.asarray(a[0], np.float64).ravel(), np.asarray(a[1], np.float64).ravel()
    bR, bt = np.asarray(b[0], np.float64).ravel(), np.asarray(b[1], np.float64).ravel()
    with np.errstate(all="ignore"):
        R = np.array([((aR[3 * i] * bR[j]) + (aR[3 * i + 1] * bR[3 + j])) + (aR[3 * i + 2] * bR[6 + j]) for i in range(3) for j in range(3)])
        t = np.array([(((aR[3 * i] * bt[0]) + (aR[3 * i + 1] * bt[1])) + (aR[3 * i + 2] * bt[2])) + at[i] for i in range(3)])
    return R, t


def align(camera, opt, guess, disp_model, normals_model, disp_new):
    """pm_align_disparity -> ((R[9], t[3]), info) with info = dict(valid, n_model, n_gate, n_used, iterations, rms_px, H[21])."""
    start = (np.asarray((guess or IDENTITY)[0], np.float64).ravel().copy(), np.asarray((guess or IDENTITY)[1], np.float64).ravel().copy())
    m, failed, done = start, False, 0
    for _ in range(opt["iterations"]):
        ev = evaluate(camera, opt, m, disp_model, normals_model, disp_new)
        ok, m2, delta = step(ev["H"], ev["g"], m)
        if not ok:
            failed = True
            break
        m = m2
        done += 1
        biggest = 0.0
        for v in delta:  # as the loop in C: a NaN is never the biggest
            biggest = abs(v) if abs(v) > biggest else biggest
        if biggest < opt["epsilon"]:
            break
    ev = evaluate(camera, opt, m, disp_model, normals_model, disp_new)
    valid = (not failed) and ev["n_used"] >= opt["min_used"]
    with np.errstate(all="ignore"):
        rms = float(np.sqrt(ev["rr"] / np.float64(ev["n_used"]))) if ev["n_used"] else 0.0
    info = dict(valid=int(valid), n_model=ev["n_model"], n_gate=ev["n_gate"], n_used=ev["n_used"], iterations=done, rms_px=rms,
                H=ev["H"])
    return (m if valid else start), info
