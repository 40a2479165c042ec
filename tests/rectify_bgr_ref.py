"""The CPU definition of undistortion + rectification of interleaved 8-bit BGR images (include/pm/imaging.h:
pm_rectify_bgr8, pm_match_raw_bgr_device), in numpy.  The kernel (csrc/pm_rectify.hpp: rectify_four) is held to it bit
for bit.

It is the gray definition (tests/rectify_ref.py) channel by channel at the SAME Q5 coordinates:
  out[..., c], valid = remap_q5(src[..., c], source_q5(view, rows, cols), border_value)        c = 0, 1, 2
border_value is one value for the three channels.  valid is one mask per image: whether a tap lies inside the source
depends on the position alone, so the three channels' masks are identical by construction -- asserted below.  The map is
the gray one, unchanged.

The optional float image is CastImage3bTo3f (image_util.cpp:25-31), the form the range-dependent stages take:
  out_f = float32(out) * float32(1.0 / 255.0)                  ONE binary32 multiplication per value
"""
import numpy as np

import rectify_ref as RR

INV255 = np.float32(1.0 / 255.0)


def remap_bgr(src, xy, border_value=0):
    """One image [src_rows][src_cols][3] uint8 at the Q5 coordinates xy -> (out [rows][cols][3] uint8, valid [rows][cols])."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    planes = [RR.remap_q5(np.ascontiguousarray(src[:, :, c]), xy, border_value) for c in range(3)]
    valid = planes[0][1]
    assert all(np.array_equal(p[1], valid) for p in planes)  # one mask per image
    return np.stack([p[0] for p in planes], axis=-1), valid


def to_float(out):
    """uint8 -> float32, x (float)(1 / 255.): one binary32 multiplication."""
    out = np.asarray(out)
    assert out.dtype == np.uint8
    return out.astype(np.float32) * INV255


def rectify_bgr(src, view, rows, cols, border_value=0):
    """pm_rectify_bgr8 of one image ([src_rows][src_cols][3] uint8) or of n images ([n][src_rows][src_cols][3])
    -> (out, out_f, valid, xy)."""
    src = np.asarray(src)
    xy = RR.source_q5(view, rows, cols)
    if src.ndim == 3:
        out, valid = remap_bgr(src, xy, border_value)
    else:
        pairs = [remap_bgr(s, xy, border_value) for s in src]
        out, valid = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return out, to_float(out), valid, xy
