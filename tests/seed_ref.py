"""The seeder's stages between the oracle's functions, in numpy and Python ints (tests/test_seed_stages.py).

oracle/pm_seed_oracle.c defines the corner response (corner_response_map), the detector as a whole (gftt_detect), the
matcher (match_rectified) and the dilation (dilate_rect).  The device runs the detector as three launches -- candidates,
selection -- and the scatter + dilation + resize as its splat; what each must deliver is restated here, and the CPU
tests of test_seed_stages.py pin the restatement to the oracle's composed functions.
"""
import numpy as np

import oracle_lib as oracle


def key_of(value, y, x):
    """A candidate key as the suppression kernel writes it: float bits << 32 | y << 16 | x."""
    return (int(np.float32(value).view(np.uint32)) << 32) | (int(y) << 16) | int(x)


def key_xy(key):
    return int(key) & 0xffff, (int(key) >> 16) & 0xffff


def max_bits(response):
    """The maximum of the positive responses as float bits; 0 where none is positive (pmo_gftt_detect's maxv)."""
    m = np.float32(max(float(np.max(response)), 0.0)) if response.size else np.float32(0)
    return int(m.view(np.uint32))


def threshold(maxv, quality):
    """(float)((double)maxv * quality_level), pmo_gftt_detect's thr."""
    return np.float32(np.float64(np.float32(maxv)) * np.float64(quality))


def candidates(response, quality):
    """The key set of the candidates: strictly above the threshold, a (non-strict) maximum of its 3 x 3 neighbourhood,
    not on the border ring."""
    r = np.asarray(response, dtype=np.float32)
    rows, cols = r.shape
    if rows < 3 or cols < 3:
        return set()
    thr = threshold(np.uint32(max_bits(r)).view(np.float32), quality)
    c = r[1:-1, 1:-1]
    ok = c > thr
    for j in range(3):
        for i in range(3):
            ok &= ~(r[j:j + rows - 2, i:i + cols - 2] > c)
    ys, xs = np.nonzero(ok)
    return {key_of(c[y, x], y + 1, x + 1) for y, x in zip(ys.tolist(), xs.tolist())}


def greedy_select(keys, min_distance, max_features):
    """cv::goodFeaturesToTrack's loop: candidates in descending 64-bit key order (strongest first, ties to the larger
    y << 16 | x); one is accepted iff no accepted corner is closer than min_distance (strict <; min_distance < 1 accepts
    all); stops at max_features -> [(x, y)]."""
    md2 = int(min_distance) * int(min_distance)
    ax, ay, out = np.zeros(max(max_features, 1), np.int64), np.zeros(max(max_features, 1), np.int64), []
    for key in sorted((int(k) for k in keys), reverse=True):
        if len(out) >= max_features:
            break
        x, y = key_xy(key)
        n = len(out)
        if min_distance >= 1 and n and bool(np.any((ax[:n] - x) ** 2 + (ay[:n] - y) ** 2 < md2)):
            continue
        ax[n], ay[n] = x, y
        out.append((x, y))
    return out


def nearest_resize(full, out_rows, out_cols):
    """cv::resize(INTER_NEAREST) as tests/test_seed.py::test_cpu_initialize_known_answers states it."""
    rows, cols = full.shape
    ys = np.minimum(np.floor(np.arange(out_rows) * (1.0 / (out_rows / rows))).astype(int), rows - 1)
    xs = np.minimum(np.floor(np.arange(out_cols) * (1.0 / (out_cols / cols))).astype(int), cols - 1)
    return full[ys][:, xs]


def splat(xy, d, rows, cols, k, inv_scale=1.0, dedup=True, out_shape=None):
    """The scatter disps(y, x) = d of the corners with d >= 0 that lie in the image, in order, so that the last one owns
    a pixel (dedup; without it -- integer corners, which cannot coincide -- the largest does), oracle.dilate_rect with
    half-width k, the nearest resize to out_shape and the scale (a power of two: exact, so it commutes with the rest)."""
    assert np.frexp(inv_scale)[0] == 0.5, "powers of two only"
    sparse = np.zeros((rows, cols), np.float32)
    for (x, y), v in zip(np.asarray(xy).reshape(-1, 2).tolist(), np.asarray(d, dtype=np.float32).tolist()):
        if v >= 0 and 0 <= x < cols and 0 <= y < rows:
            sparse[y, x] = v if dedup else max(sparse[y, x], v)
    full = oracle.dilate_rect(sparse, k)
    if out_shape is not None and tuple(out_shape) != (rows, cols):
        full = nearest_resize(full, *out_shape)
    return np.ascontiguousarray(full * np.float32(inv_scale))
