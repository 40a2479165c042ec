"""The CPU definition of the fast guided filter with a one-channel guide (include/pm/imaging.h:
pm_fast_guided_filter, pm_estimate_illuminant_range_guided), in numpy.

It follows the reference's src/vehicle/imaging/fast_guided_filter.cpp (FastGuidedFilterMono, :90-123; filter(),
:68-87; fastGuidedFilter(), :207-233) operation by operation: every cv::Mat operation is one IEEE binary32 rounding
per element, nothing is contracted.  The OpenCV primitives it rests on (cv::resize INTER_NN / INTER_LINEAR on
floats, cv::blur with BORDER_REFLECT_101) are restated here; this restatement is THIS PROJECT'S definition of
them ("still assumed"): the reference tree holds no expected outputs for them and cannot be
compiled without OpenCV.  Where OpenCV leaves an order open -- cv::blur accumulates float images in binary64, in an
order that depends on its SIMD path -- the definition FIXES one, so that a device can reproduce it bit for bit:

  box mean, k x k, per output pixel: the k taps of a row are added left to right in binary64 (starting from 0.0),
  then the k row sums top to bottom in binary64 (starting from 0.0), times 1.0 / (k * k) in binary64, one rounding
  to binary32.

numpy's own sum / cumsum are pairwise, so the taps are looped over explicitly (vectorised over pixels).
"""
import numpy as np

f32 = np.float32


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101), including its repeated reflection when |p| >= n."""
    p = np.array(p, dtype=np.int64, copy=True)
    if n == 1:
        return np.zeros_like(p)
    while True:
        neg, big = p < 0, p >= n
        if not (neg.any() or big.any()):
            return p
        p = np.where(neg, -p, np.where(big, 2 * n - 2 - p, p))


def nn_index(dst, src):
    """cv::resize INTER_NN source index of every destination index along one axis."""
    inv = 1.0 / (float(dst) / float(src))
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * inv).astype(np.int64), src - 1)


def resize_nn(img, rows, cols):
    return img[nn_index(rows, img.shape[0])][:, nn_index(cols, img.shape[1])]


def box_mean(plane, k):
    """cv::blur(plane, Size(k, k)) of a binary32 plane in the fixed order of the module's head."""
    assert plane.dtype == np.float32 and plane.ndim == 2 and k >= 1 and k % 2 == 1
    H, W = plane.shape
    p64 = plane.astype(np.float64)
    wide = p64[:, reflect101(np.arange(-(k // 2), W + k // 2), W)]
    rowsum = np.zeros((H, W), np.float64)
    for i in range(k):  # left to right
        rowsum = rowsum + wide[:, i:i + W]
    tall = rowsum[reflect101(np.arange(-(k // 2), H + k // 2), H)]
    total = np.zeros((H, W), np.float64)
    for j in range(k):  # top to bottom
        total = total + tall[j:j + H]
    return (total * (1.0 / (k * k))).astype(np.float32)


def linear_axis(dst, src):
    """cv::resize INTER_LINEAR on floats, one axis: (index of the left tap, binary32 weight of the right tap)."""
    scale = 1.0 / (float(dst) / float(src))
    fx = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    i = np.floor(fx).astype(np.int64)
    fx = (fx - i.astype(np.float32)).astype(np.float32)
    low, high = i < 0, i >= src - 1
    fx = np.where(low | high, f32(0), fx).astype(np.float32)
    i = np.where(low, 0, np.where(high, src - 1, i))
    return i, fx


def resize_linear(plane, rows, cols):
    assert plane.dtype == np.float32
    H, W = plane.shape
    ix, fx = linear_axis(cols, W)
    iy, fy = linear_axis(rows, H)
    one = f32(1)
    ix1 = np.minimum(ix + 1, W - 1)
    hor = (plane[:, ix] * (one - fx)[None, :]).astype(np.float32) + (plane[:, ix1] * fx[None, :]).astype(np.float32)
    hor = hor.astype(np.float32)
    iy1 = np.minimum(iy + 1, H - 1)
    ver = (hor[iy] * (one - fy)[:, None]).astype(np.float32) + (hor[iy1] * fy[:, None]).astype(np.float32)
    return ver.astype(np.float32)


def coarse_size(rows, cols, s):
    return rows // s, cols // s


def box_size(r, s):
    return 2 * (r // s) + 1


def fast_guided_filter(guide, src, r, eps, s, scale=1.0):
    """fastGuidedFilter(I = guide, p = src, r, eps, s) * scale.  guide: (rows, cols) binary32; src: (rows, cols) or
    (rows, cols, channels) binary32, each channel filtered on its own."""
    guide = np.ascontiguousarray(guide, np.float32)
    src = np.ascontiguousarray(src, np.float32)
    rows, cols = guide.shape
    assert src.shape[:2] == (rows, cols) and s >= 1 and r >= 0 and rows // s >= 1 and cols // s >= 1
    squeeze = src.ndim == 2
    if squeeze:
        src = src[:, :, None]
    k = box_size(r, s)
    ch, cw = coarse_size(rows, cols, s)
    with np.errstate(all="ignore"):
        I = resize_nn(guide, ch, cw)
        mean_I = box_mean(I, k)
        mean_II = box_mean(I * I, k)
        var_I = mean_II - mean_I * mean_I
        out = np.empty_like(src)
        for c in range(src.shape[2]):
            p = resize_nn(src[:, :, c], ch, cw)
            mean_p = box_mean(p, k)
            mean_Ip = box_mean(I * p, k)
            cov_Ip = mean_Ip - mean_I * mean_p
            a = cov_Ip / (var_I + f32(eps))
            b = mean_p - a * mean_I
            mean_a = resize_linear(box_mean(a, k), rows, cols)
            mean_b = resize_linear(box_mean(b, k), rows, cols)
            out[:, :, c] = (mean_a * guide + mean_b) * f32(scale)
    assert out.dtype == np.float32
    return out[:, :, 0] if squeeze else out


def estimate_illuminant_range_guided(bgr, range_map, r, eps, s):
    """EstimateIlluminantRangeGuided (illuminant.cpp:24-34): 2.0f * fastGuidedFilter(range, bgr, r, eps, s)."""
    return fast_guided_filter(range_map, bgr, r, eps, s, scale=2.0)


def next_even_int(x):
    """core::NextEvenInt (math_util.hpp): x + x % 2."""
    return x + (x % 2)


def reference_parameters(cols):
    """EnhanceUnderwater's setting (enhance.cpp:60-62): r, eps, s."""
    return next_even_int(cols // 3), 0.01, 8
