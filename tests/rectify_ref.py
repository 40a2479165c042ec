"""The CPU definition of undistortion + rectification (include/pm/imaging.h: pm_rectify_u8, pm_rectify_map,
pm_match_raw_device), in numpy.  The kernel (csrc/pm_rectify.hpp) is held to it bit for bit.

It is THIS PROJECT'S definition.  The reference has no such stage: it ships a calibration with non-zero distortion
(config/shared/ACFR.yaml:27,48) and warns that it does not undistort (src/vehicle/params/yaml_parser.cpp:153).  OpenCV's
remap is not restated either: its 15-bit coefficient table is not reproduced and nothing here claims parity with it.

A view is 22 binary64 numbers in the order of pm_rectify_view:
  cam = (fx, fy, cx, cy, k1, k2, p1, p2, k3)   the raw camera, radial-tangential model
  R[9]                                          row-major, x_rect = R x_raw
  (fx', fy', cx', cy')                          the pinhole of the rectified image

Geometry, per destination pixel (u, v): binary64, ONE rounding per operation, in exactly this order (numpy evaluates
every elementwise operation on its own, nothing is contracted):
  a = (u - cx') / fx'            b = (v - cy') / fy'
  X = (R00*a + R10*b) + R20      Y = (R01*a + R11*b) + R21      W = (R02*a + R12*b) + R22        # R^T (a, b, 1)
  not (W > 0): INVALID
  x = X / W   y = Y / W   xx = x*x   yy = y*y   xy = x*y   r2 = xx + yy
  rad = 1 + r2*(k1 + r2*(k2 + r2*k3))
  tx  = ((2*p1)*xy) + (p2*(r2 + (2*xx)))
  ty  = (p1*(r2 + (2*yy))) + ((2*p2)*xy)
  sx  = fx*((x*rad) + tx) + cx   sy = fy*((y*rad) + ty) + cy
  qx  = sx*32    qy = sy*32
  not (|qx| < 2^30 and |qy| < 2^30): INVALID                    # also NaN / inf
  ix = rint(qx)  iy = rint(qy)                                  # round half to even, int32
Interpolation, integer: x0 = ix >> 5 (floor), ax = ix & 31, likewise y0, ay; taps (x0,y0) (x0+1,y0) (x0,y0+1)
(x0+1,y0+1) with weights (32-ax)(32-ay), ax(32-ay), (32-ax)ay, ax*ay; a tap outside the source reads border_value;
out = (sum of w*p + 512) >> 10; valid = 255 iff every tap with a non-zero weight lies inside the source, else 0.
An INVALID pixel: out = border_value, valid = 0, map entry (INT32_MIN, INT32_MIN).
"""
import numpy as np

INVALID = np.iinfo(np.int32).min
Q = 32          # positions are quantised to 1 / 32 pixel (Q5)
LIMIT = 2.0 ** 30


def make_view(cam, R, pinhole):
    """cam: 9 numbers, R: 3x3 (or 9, row-major), pinhole: (fx', fy', cx', cy') -> the 22 doubles of pm_rectify_view."""
    v = np.concatenate([np.asarray(cam, np.float64).reshape(9), np.asarray(R, np.float64).reshape(9),
                        np.asarray(pinhole, np.float64).reshape(4)])
    assert v.shape == (22,)
    return v


def identity_view(fx, fy, cx, cy):
    return make_view([fx, fy, cx, cy, 0, 0, 0, 0, 0], np.eye(3), [fx, fy, cx, cy])


def source_q5(view, rows, cols):
    """The Q5 source coordinates of every destination pixel: int32 [rows][cols][2] (x, y), INVALID twice where the
    pixel has no source position."""
    view = np.asarray(view, np.float64)
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = view[:9]
    R = view[9:18]
    fxn, fyn, cxn, cyn = view[18:]
    u = np.arange(cols, dtype=np.float64)[None, :]
    v = np.arange(rows, dtype=np.float64)[:, None]
    two = np.float64(2.0)
    with np.errstate(all="ignore"):
        a = np.broadcast_to((u - cxn) / fxn, (rows, cols))
        b = np.broadcast_to((v - cyn) / fyn, (rows, cols))
        X = (R[0] * a + R[3] * b) + R[6]
        Y = (R[1] * a + R[4] * b) + R[7]
        W = (R[2] * a + R[5] * b) + R[8]
        x = X / W
        y = Y / W
        xx = x * x
        yy = y * y
        xy = x * y
        r2 = xx + yy
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        tx = ((two * p1) * xy) + (p2 * (r2 + (two * xx)))
        ty = (p1 * (r2 + (two * yy))) + ((two * p2) * xy)
        sx = fx * ((x * rad) + tx) + cx
        sy = fy * ((y * rad) + ty) + cy
        qx = sx * 32.0
        qy = sy * 32.0
        ok = (W > 0) & (np.abs(qx) < LIMIT) & (np.abs(qy) < LIMIT)
        ix = np.rint(np.where(ok, qx, 0.0)).astype(np.int64)
        iy = np.rint(np.where(ok, qy, 0.0)).astype(np.int64)
    out = np.empty((rows, cols, 2), np.int32)
    out[:, :, 0] = np.where(ok, ix, INVALID)
    out[:, :, 1] = np.where(ok, iy, INVALID)
    return out


def remap_q5(src, xy, border_value=0):
    """The integer interpolation of one image at the Q5 coordinates xy -> (out uint8, valid uint8)."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2 and 0 <= border_value <= 255
    H, W = src.shape
    ix = xy[:, :, 0].astype(np.int64)
    iy = xy[:, :, 1].astype(np.int64)
    ok = (xy[:, :, 0] != INVALID) | (xy[:, :, 1] != INVALID)
    x0, y0 = ix >> 5, iy >> 5
    ax, ay = ix & 31, iy & 31
    total = np.zeros(ix.shape, np.int64)
    all_in = ok.copy()
    for dx, dy, w in ((0, 0, (Q - ax) * (Q - ay)), (1, 0, ax * (Q - ay)), (0, 1, (Q - ax) * ay), (1, 1, ax * ay)):
        tx, ty = x0 + dx, y0 + dy
        inside = ok & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        p = np.where(inside, src[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)].astype(np.int64), border_value)
        total += w * p
        all_in &= inside | (w == 0)
    out = np.where(ok, (total + 512) >> 10, border_value).astype(np.uint8)
    return out, np.where(all_in, 255, 0).astype(np.uint8)


def rectify(src, view, rows, cols, border_value=0):
    """pm_rectify_u8 of one image (2-D uint8) or of n images ([n][src_rows][src_cols]) -> (out, valid, xy)."""
    src = np.asarray(src)
    xy = source_q5(view, rows, cols)
    if src.ndim == 2:
        out, valid = remap_q5(src, xy, border_value)
        return out, valid, xy
    pairs = [remap_q5(s, xy, border_value) for s in src]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), xy
