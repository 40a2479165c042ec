"""The definition of pm_disparity_confidence (include/pm/imaging.h): how well each disparity of a left map matched, told by four
evaluations of the matching functor around the answer and the left-right residual.  It is built on the pinned oracle
(tests/oracle_lib.py) and shares nothing with the kernels; the device is held to it with tolerance 0, bit patterns compared.

  G_l, G_r  oracle_lib.gradient_magnitude of the two images.
  cost(d)   oracle_lib.cpu_cost(ims, pw, ph, x, y, d, literal=False) under the functor (alpha, tau_color, tau_grad).
Every operation below is ONE binary32 rounding unless it says binary64.
  interior  pw / 2 <= x <= cols - pw / 2 - 1 and ph / 2 <= y <= rows - ph / 2 - 1; empty where the window does not fit.
  valid     d = D_l(y, x) > 0: not for 0, -0.0, negatives and NaN.
  MEASURED  valid, interior and d <= hi, hi = (float)x - (float)(pw / 2): the domain in which pmo_cpu_cost_direct's two-tap
            form holds.  +inf and values beyond hi are valid but not measured; nothing is clamped.
  costs     c0 = cost(d); c_bg = cost(+0.0f); dm = d - 1.0f, side M exists iff dm >= 0, cm = cost(dm); dp = d + 1.0f, side P
            exists iff dp <= hi, cp = cost(dp).
  margin    both sides: cn = cp < cm ? cp : cm, margin = cn - c0; one side: that side's cost - c0; no side: +0.0f.
  bg_margin c_bg - c0.
  lr        with D_r: q = (int)fmaxf((float)x - d, 0.f); r = D_r(y, q); r > 0: (float)fabs((double)r - (double)d), else +inf.
            Without D_r: +inf, and FAIL_LR is never set.
  flags     measured: MEASURED | FAIL_COST unless c0 <= max_cost | FAIL_MARGIN unless margin >= min_margin | FAIL_BG unless
            bg_margin >= min_bg_margin | (with D_r) FAIL_LR unless lr <= max_lr_diff.  Not measured: 0.  KEPT iff flags == MEASURED.
  out       a measured pixel that is not KEPT becomes +0.0f; with drop_unmeasured so does a valid pixel that is not measured;
            every other pixel keeps its input BITS.
  measures  [4][rows][cols]: c0, margin, bg_margin, lr; a pixel that is not measured gets -1.0f, +0.0f, +0.0f, +inf.
  counts    int32 [valid, measured, kept].
"""
import numpy as np

import oracle_lib as O

MEASURED, FAIL_COST, FAIL_MARGIN, FAIL_BG, FAIL_LR = 1, 2, 4, 8, 16
F = np.float32


def confidence(left, right, disp_l, disp_r=None, pw=5, ph=5, max_cost=np.inf, min_margin=-np.inf, min_bg_margin=-np.inf,
               max_lr_diff=np.inf, drop_unmeasured=0, functor=(0.7, 50.0, 20.0)):
    """-> dict(out, measures [4][rows][cols], flags uint8, counts int32[3], valid, measured, kept (bool maps),
    sides (int8: existing sides of a measured pixel, -1 elsewhere))."""
    disp_l = np.ascontiguousarray(disp_l, np.float32)
    rows, cols = disp_l.shape
    ims = O.ImageSet(left, right)
    f = O.functor(*functor)
    cost = lambda x, y, d: F(O.cpu_cost(ims, pw, ph, x, y, F(d), literal=False, f=f))
    thr = [F(max_cost), F(min_margin), F(min_bg_margin), F(max_lr_diff)]
    out = disp_l.copy()
    meas = np.empty((4, rows, cols), np.float32)
    meas[0], meas[1], meas[2], meas[3] = F(-1.0), F(0.0), F(0.0), F(np.inf)
    flags = np.zeros((rows, cols), np.uint8)
    sides = np.full((rows, cols), -1, np.int8)
    with np.errstate(invalid="ignore"):
        valid = disp_l > 0
    measured = np.zeros((rows, cols), bool)
    for y in range(ph // 2, rows - ph // 2):
        for x in range(pw // 2, cols - pw // 2):
            d = disp_l[y, x]
            hi = F(x) - F(pw // 2)
            if not (valid[y, x] and d <= hi):
                continue
            measured[y, x] = True
            c0, c_bg = cost(x, y, d), cost(x, y, F(0.0))
            dm, dp = F(d - F(1.0)), F(d + F(1.0))
            has_m, has_p = bool(dm >= 0), bool(dp <= hi)
            cm = cost(x, y, dm) if has_m else None
            cp = cost(x, y, dp) if has_p else None
            if has_m and has_p:
                margin = F((cp if cp < cm else cm) - c0)
            elif has_m:
                margin = F(cm - c0)
            elif has_p:
                margin = F(cp - c0)
            else:
                margin = F(0.0)
            bg_margin = F(c_bg - c0)
            lr = F(np.inf)
            if disp_r is not None:
                q = int(max(F(F(x) - d), F(0.0)))
                r = F(disp_r[y, q])
                if r > 0:
                    with np.errstate(over="ignore"):
                        lr = F(abs(np.float64(r) - np.float64(d)))
            fl = MEASURED
            fl |= 0 if c0 <= thr[0] else FAIL_COST
            fl |= 0 if margin >= thr[1] else FAIL_MARGIN
            fl |= 0 if bg_margin >= thr[2] else FAIL_BG
            if disp_r is not None:
                fl |= 0 if lr <= thr[3] else FAIL_LR
            flags[y, x] = fl
            sides[y, x] = int(has_m) + int(has_p)
            meas[:, y, x] = (c0, margin, bg_margin, lr)
    kept = flags == MEASURED
    out[measured & ~kept] = F(0.0)
    if drop_unmeasured:
        out[valid & ~measured] = F(0.0)
    counts = np.array([valid.sum(), measured.sum(), kept.sum()], np.int32)
    return dict(out=out, measures=meas, flags=flags, counts=counts, valid=valid, measured=measured, kept=kept, sides=sides)
