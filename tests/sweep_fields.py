"""Crafted image pairs and disparity fields for ONE sweep observed on its own (pm_propagate / pm_debug_propagate): what
the stage tests of tests/test_gpu_parity.py and the variant tests of tests/test_sweep_variants.py run the sweep kernels
on.  Every builder is a pure function of its arguments (seeded generators), so two tests that ask for the same field get
the same field; the defaults are the shapes tests/test_gpu_parity.py has always used."""
import numpy as np

from conftest import small_pair

GPU_ADVERSARIAL_KINDS = ["random", "plateaus", "huge", "tiny"]


def weight_extremes(synth, pw, rows=40, cols=200):
    """PM_SEM_CPU: sample positions within a few ulps of an integer column -- the fixed-point lerp weights reach 0 and
    65536 on both sides of the integer -- next to ordinary fractions and runs of three equal values.
    -> (left, right, disparity)"""
    l, r, _, _, _ = small_pair(synth, 23, rows, cols, n_points=20, dilate_factor=2)
    rng = np.random.default_rng(17)
    xs = np.arange(cols, dtype=np.float32)[None, :].repeat(rows, 0)
    shift = np.float32((pw - 1) * 0.5)
    # x - d - shift = k + eps  with  eps in {0, +-1 ulp ... +-2^-16, +-2^-17, +-2^-18}
    k = rng.integers(0, 60, (rows, cols)).astype(np.float32)
    eps = rng.choice(np.array([0.0, 2.0 ** -16, -2.0 ** -16, 2.0 ** -17, -2.0 ** -17, 2.0 ** -18, -2.0 ** -18, 7.6e-6,
                               -7.6e-6, 7.7e-6, -7.7e-6, 0.25, 0.5], np.float32), (rows, cols))
    d = np.maximum(xs - shift - k - eps, 0).astype(np.float32)
    d = np.repeat(d[:, ::3], 3, axis=1)[:, :cols]        # runs of three equal values
    d[rng.random((rows, cols)) < 0.3] = np.float32(13.99999)
    return l, r, d


RUN_VALUE = 6.0  # the disparity that runs along the chains of one_value_runs(): the pair's true shift


def one_value_runs(pw, layout, rows=None, cols=None):
    """PM_SEM_CPU: ONE value runs along whole chains.  The right image is the left one shifted by RUN_VALUE pixels, the
    map is wrong everywhere except for one pixel per chain that holds RUN_VALUE -- at the chain's first position,
    somewhere in the middle, or not at all -- and a stretch without texture stops the run (every candidate costs the same
    there, and the rule is a strict <).  layout "rows": the value runs along the rows, "cols": along the columns; the
    stretch without texture lies a third (rows) / four ninths (cols) of the way along the chains, in the chains from 14
    (rows) / 30 (cols) on, where the image has that many.  -> (left, right, disparity)"""
    if rows is None:
        rows, cols = (22, 900) if layout == "rows" else (900, 52)
    rng = np.random.default_rng(23)
    l = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    if layout == "rows":
        stop = cols // 3
        l[14:, stop:stop + min(30, cols // 10)] = 77   # no texture: the run stops here in the lower rows
    else:
        stop = 4 * rows // 9
        l[stop:stop + min(30, rows // 10), 30:] = 77
    r = np.roll(l, -int(RUN_VALUE), axis=1)           # left (x) = right (x - 6)
    d = rng.uniform(8.0, 40.0, (rows, cols)).astype(np.float32)
    h = pw // 2
    if layout == "rows":
        d[:8, h] = RUN_VALUE                # from the first position of the forward sweep
        d[4:12, cols - 1 - h] = RUN_VALUE   # ... and of the backward sweep
        for y in range(12, rows):
            d[y, rng.integers(h, cols - h)] = RUN_VALUE
    else:
        d[h, 7:25] = RUN_VALUE
        d[rows - 1 - h, 20:40] = RUN_VALUE
        for x in range(40, cols):
            d[rng.integers(h, rows - h), x] = RUN_VALUE
    return l, r, d


def gpu_adversarial(synth, kind, rows=45, cols=333):
    """PM_SEM_GPU: fields that exercise the clamp (x - d < 1), the single-position slow path, long runs of one value and
    binade crossings of the sample positions.  -> (left, right, disparity)"""
    l, r, _, _, _ = small_pair(synth, 21, rows, cols, n_points=20, dilate_factor=2)
    rng = np.random.default_rng(5)
    if kind == "random":
        d = rng.uniform(0.0, 90.0, (rows, cols)).astype(np.float32)
    elif kind == "plateaus":
        d = np.repeat(np.repeat(rng.uniform(0.0, 40.0, (rows // 5 + 1, cols // 9 + 1)), 5, 0), 9, 1)
        d = d[:rows, :cols].astype(np.float32)
        d[rng.random((rows, cols)) < 0.05] = 0.0
    elif kind == "huge":  # mostly clamped candidates
        d = rng.uniform(100.0, 600.0, (rows, cols)).astype(np.float32)
        d[:, ::7] = 3.25
    elif kind == "tiny":  # values around powers of two of x - d, and denormal-small disparities
        xs = np.arange(cols, dtype=np.float32)[None, :].repeat(rows, 0)
        pick = rng.choice(np.array([1, 2, 4, 8, 16, 32, 64, 128], np.float32), (rows, cols))
        d = np.maximum(xs - pick + rng.choice(np.array([-1e-3, 0, 1e-3, 0.5], np.float32), (rows, cols)), 0)
        d[rng.random((rows, cols)) < 0.1] = 1e-30
        d = d.astype(np.float32)
    else:
        raise ValueError(kind)
    return l, r, d
