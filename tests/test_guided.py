"""The fast guided filter with a one-channel guide, EstimateIlluminantRangeGuided on top of it, and the pixel gather
(include/pm/imaging.h: pm_fast_guided_filter, pm_estimate_illuminant_range_guided, pm_gather_pixels).

CPU tests pin the definition (tests/guided_ref.py): known answers by hand, independent binary64 implementations
(scipy's uniform_filter, a straightforward guided filter built from it), and a fixture the definition wrote.
GPU tests hold the kernels to the definition with tolerance 0: every operation of the definition is a single IEEE
rounding in a fixed order, the build uses -ffp-contract=off and correctly rounded division."""
import os
import subprocess

import numpy as np
import pytest

import guided_ref as G
import oracle_lib as O
from conftest import GOLDEN
from cpp_build import build_caller
from test_imaging import B0, BETA_B0, X0, RTOL, ATOL, scene

FIXTURE = os.path.join(GOLDEN, "guided_61x99.npz")
FX, BASELINE = 415.876509, 0.12


def range_scene(rows, cols, seed):
    """Guide and source built like tests/test_imaging.py::scene: a range map with about 20 % zeros (no range) and a
    uniform colour image."""
    bgr, disp = scene(rows, cols, seed)
    return O.disp_to_range(disp, FX, BASELINE), bgr


def smooth_guide(rows, cols):
    y, x = np.mgrid[0:rows, 0:cols]
    return (2.0 + 1.5 * np.sin(x / 7.0) + 1.2 * np.cos(y / 5.0) + 0.01 * x).astype(np.float32)


# ---- independent binary64 implementations (written apart from guided_ref.py) -----------------------------------
def box64(plane, k):
    from scipy.ndimage import uniform_filter
    return uniform_filter(np.asarray(plane, np.float64), size=k, mode="mirror")


def guided64(guide, src, r, eps, s):
    """A straightforward binary64 fast guided filter: He & Sun's algorithm on scipy's box mean, the same nearest /
    bilinear index rules as OpenCV.  Only valid where k / 2 < both coarse dimensions (scipy reflects once)."""
    rows, cols = guide.shape
    ch, cw = rows // s, cols // s
    k = 2 * (r // s) + 1
    assert k // 2 < ch and k // 2 < cw
    ys = [min(int(np.floor(y * (1.0 / (ch / rows)))), rows - 1) for y in range(ch)]
    xs = [min(int(np.floor(x * (1.0 / (cw / cols)))), cols - 1) for x in range(cw)]
    I = guide.astype(np.float64)[np.ix_(ys, xs)]
    mI = box64(I, k)
    var = box64(I * I, k) - mI * mI

    def taps(dst, n):
        pos = (np.arange(dst) + 0.5) * (1.0 / (dst / n)) - 0.5
        i = np.floor(pos).astype(int)
        w = pos - i
        w[(i < 0) | (i >= n - 1)] = 0.0
        i = np.clip(i, 0, n - 1)
        return i, np.minimum(i + 1, n - 1), w

    x0, x1, wx = taps(cols, cw)
    y0, y1, wy = taps(rows, ch)

    def up(m):
        hor = m[:, x0] * (1 - wx) + m[:, x1] * wx
        return hor[y0] * (1 - wy)[:, None] + hor[y1] * wy[:, None]

    out = np.empty(src.shape, np.float64)
    for c in range(src.shape[2]):
        p = src[:, :, c].astype(np.float64)[np.ix_(ys, xs)]
        mp = box64(p, k)
        a = (box64(I * p, k) - mI * mp) / (var + eps)
        b = mp - a * mI
        out[:, :, c] = up(box64(a, k)) * guide + up(box64(b, k))
    return out


def rel_diff(got, want):
    """Largest difference relative to the scale of the expected image."""
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want)) / np.max(np.abs(want)))


BOX_CASES = [(90, 160, 107), (30, 47, 31), (61, 99, 11), (15, 24, 5)]
FILTER_CASES = [  # rows, cols, r, eps, s, guide kind
    (61, 99, 22, 0.01, 4, "range"), (48, 64, 5, 0.01, 1, "range"), (240, 322, 108, 0.01, 8, "range"),
    (240, 322, 40, 0.01, 4, "range"), (96, 160, 54, 0.01, 8, "smooth"), (37, 53, 8, 0.1, 4, "smooth"),
]
# measured on the CPU with the cases above (the figures are in the docstrings); the tests assert twice the measurement
BOX_MEASURED = 5.93e-8     # one binary32 rounding (2^-24 = 5.96e-8)
FILTER_MEASURED = 2.10e-7  # a few binary32 roundings of values of the output's size
LINEAR_MEASURED = 5.99e-7


def _filter_case(rows, cols, kind, seed):
    guide, bgr = range_scene(rows, cols, seed)
    if kind == "smooth":
        guide = smooth_guide(rows, cols)
    return guide, bgr


def measure_box():
    worst = 0.0
    for rows, cols, k in BOX_CASES:
        p = np.random.default_rng(rows + cols).uniform(0.05, 1.0, (rows, cols)).astype(np.float32)
        want = box64(p, k)
        worst = max(worst, float(np.max(np.abs(G.box_mean(p, k) - want) / np.abs(want))))
    return worst


def measure_filter():
    worst = 0.0
    for i, (rows, cols, r, eps, s, kind) in enumerate(FILTER_CASES):
        guide, bgr = _filter_case(rows, cols, kind, 100 + i)
        worst = max(worst, rel_diff(G.fast_guided_filter(guide, bgr, r, eps, s), guided64(guide, bgr, r, eps, s)))
    return worst


def measure_linear():
    worst = 0.0
    for rows, cols, s in ((96, 160, 8), (61, 99, 4), (240, 322, 8)):
        I = smooth_guide(rows, cols)
        p = (np.float32(2) * I + np.float32(3)).astype(np.float32)
        worst = max(worst, rel_diff(G.fast_guided_filter(I, p, 2 * s, 1e-6, s), p))
    return worst


# ---- 1. known answers by hand ---------------------------------------------------------------------------------
def test_index_rules_by_hand():
    assert G.reflect101(np.arange(-3, 8), 5).tolist() == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    # repeated reflection (k / 2 >= size): period 2 * (n - 1)
    assert G.reflect101(np.arange(-8, 12), 3).tolist() == [0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    assert G.reflect101(np.arange(-4, 5), 1).tolist() == [0] * 9
    assert G.nn_index(4, 9).tolist() == [0, 2, 4, 6]  # floor(x * 2.25)
    assert G.nn_index(12, 99).tolist() == [int(np.floor(x * 8.25)) for x in range(12)]
    # 2 -> 4: centres at -0.25, 0.25, 0.75, 1.25 of the source grid
    i, f = G.linear_axis(4, 2)
    assert i.tolist() == [0, 0, 0, 1] and f.tolist() == [0.0, 0.25, 0.75, 0.0]
    assert G.box_size(426, 8) == 107 and G.box_size(7, 8) == 1 and G.reference_parameters(1280) == (426, 0.01, 8)


def test_box_mean_by_hand_with_repeated_reflection():
    """Hand-indexed known answers where scipy cannot follow (it reflects once): 6 x 12 with k = 15 and 1 x 9 with
    k = 5 (a coarse dimension of 1 maps every row index to 0)."""
    rng = np.random.default_rng(5)
    for rows, cols, k in ((6, 12, 15), (1, 9, 5), (3, 2, 7)):
        p = rng.integers(0, 64, (rows, cols)).astype(np.float32)  # small integers: every sum is exact
        got = G.box_mean(p, k)

        def mirror(i, n):  # the period-2(n-1) triangle wave, written apart from reflect101
            if n == 1:
                return 0
            i = abs(i) % (2 * (n - 1))
            return i if i < n else 2 * (n - 1) - i

        for y in range(rows):
            for x in range(cols):
                total = sum(float(p[mirror(y + dy, rows), mirror(x + dx, cols)])
                            for dy in range(-(k // 2), k // 2 + 1) for dx in range(-(k // 2), k // 2 + 1))
                assert got[y, x] == np.float32(total * (1.0 / (k * k))), (rows, cols, k, y, x)


def test_constant_guide_gives_the_interpolated_box_mean():
    guide = np.full((37, 53), 3.0, np.float32)
    src = np.random.default_rng(1).uniform(0, 1, (37, 53)).astype(np.float32)
    r, eps, s = 9, 0.01, 4
    got = G.fast_guided_filter(guide, src, r, eps, s)
    p = G.resize_nn(src, 37 // s, 53 // s)
    k = G.box_size(r, s)
    smooth = G.resize_linear(G.box_mean(G.box_mean(p, k), k), 37, 53)
    # var_I = 9 - 3 * 3 = 0 exactly; cov = mean(3 p) - 3 mean(p) is 0 up to the two roundings of its terms (each
    # <= 2^-24 relative at magnitude <= 3), so |a| <= 2 * 3 * 2^-24 / eps, b = mean_p - 3 a, and the output
    # mean_a * 3 + mean_b differs from the interpolated box mean of p by at most 2 * 3 * max|a| plus roundings (1e-6)
    assert np.max(np.abs(got - smooth)) <= 6 * (6 * 2.0 ** -24 / eps) + 1e-6
    # a guide of zeros: a = 0 exactly
    got0 = G.fast_guided_filter(np.zeros((37, 53), np.float32), src, r, eps, s)
    assert np.array_equal(got0, smooth)


def test_identity_when_the_box_is_one_pixel():
    guide, bgr = range_scene(20, 33, 3)
    assert np.array_equal(G.fast_guided_filter(guide, bgr, 0, 0.01, 1), bgr)  # k = 1: var = cov = 0, a = 0, b = p
    assert np.array_equal(G.fast_guided_filter(guide, bgr[:, :, 0], 0, 0.01, 1), bgr[:, :, 0])
    assert np.array_equal(G.estimate_illuminant_range_guided(bgr, guide, 0, 0.01, 1), np.float32(2) * bgr)


def test_linear_source_is_reproduced():
    """p = 2 I + 3 on a smooth guide whose variance is large against eps = 1e-6: a = 2, b = 3, output = p.
    Measured: largest |out - p| / max|p| over 96x160 s=8, 61x99 s=4, 240x322 s=8 (r = 2 s): 5.99e-7 (LINEAR_MEASURED);
    asserted: twice that."""
    got = measure_linear()
    print("linear source: measured %.3e" % got)
    assert got <= 2 * LINEAR_MEASURED


# ---- 2. independent implementations ---------------------------------------------------------------------------
def test_box_mean_against_scipy_uniform_filter():
    """Only where k / 2 < both dimensions (scipy reflects once).  Measured: largest elementwise relative difference
    5.93e-8 (one binary32 rounding) over 90x160 k=107, 30x47 k=31, 61x99 k=11, 15x24 k=5; asserted: twice that."""
    got = measure_box()
    print("box mean vs scipy: measured %.3e" % got)
    assert got <= 2 * BOX_MEASURED


def test_whole_filter_against_binary64_guided_filter():
    """Measured: largest |definition - binary64| / max|binary64| over FILTER_CASES = 2.10e-7 (per case 9.9e-8,
    8.3e-8, 1.95e-7, 1.91e-7, 2.09e-7, 1.36e-7); asserted: twice that."""
    got = measure_filter()
    print("whole filter vs binary64: measured %.3e" % got)
    assert got <= 2 * FILTER_MEASURED


# ---- 3. the fixture the definition wrote ----------------------------------------------------------------------
def test_definition_reproduces_its_fixture():
    f = np.load(FIXTURE)
    r, s, eps = int(f["r"]), int(f["s"]), float(f["eps"])
    assert f["guide"].shape == (61, 99) and f["src"].shape == (61, 99, 3)
    assert np.array_equal(G.fast_guided_filter(f["guide"], f["src"], r, eps, s), f["output"])


# ---- device parity --------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _src(bgr, channels, seed):
    if channels <= 3:
        return np.ascontiguousarray(bgr[:, :, :channels])
    extra = np.random.default_rng(seed).uniform(0, 1, bgr.shape[:2] + (channels - 3,)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([bgr, extra], axis=2))


def _reference_r(cols):
    return G.reference_parameters(cols)[0]


# rows, cols, s, r, channels; per size: s in {1, 4, 8}, r from 0 up to one whose k / 2 exceeds the coarse height, the
# reference's own setting r = NextEvenInt(cols / 3), eps = 0.01, s = 8 (enhance.cpp:60-62)
DEVICE_CASES = [
    (48, 64, 1, 0, 1), (48, 64, 4, 8, 3), (48, 64, 8, _reference_r(64), 3), (48, 64, 8, 64, 4),
    (37, 53, 1, 3, 3), (37, 53, 4, 40, 1), (37, 53, 8, _reference_r(53), 3), (37, 53, 8, 0, 4),
    (61, 99, 1, 5, 1), (61, 99, 4, 22, 3), (61, 99, 8, 80, 4), (61, 99, 8, _reference_r(99), 3),
    (240, 322, 1, 4, 3), (240, 322, 4, 108, 3), (240, 322, 8, _reference_r(322), 3), (240, 322, 8, 300, 4),
    (240, 322, 4, 41, 1),
    (720, 1280, 8, _reference_r(1280), 3), (720, 1280, 4, 100, 1), (720, 1280, 1, 2, 4),
]


def _run_filter(e, guide, src, channels, r, eps, s, scale=1.0):
    import torch
    rows, cols = guide.shape
    d_g, d_p = _dev(guide), _dev(src)
    d_o = torch.empty_like(d_p)
    e.fast_guided_filter(d_g.data_ptr(), d_p.data_ptr(), rows, cols, channels, r, eps, s, scale, d_o.data_ptr())
    e.synchronize()
    return d_o.cpu().numpy().reshape(src.shape)


@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        yield e


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,s,r,channels", DEVICE_CASES)
def test_device_filter_equals_definition(engine, rows, cols, s, r, channels):
    guide, bgr = range_scene(rows, cols, rows * 3 + cols + s)
    src = _src(bgr, channels, r)
    assert (guide == 0).mean() > 0.1
    got = _run_filter(engine, guide, src, channels, r, 0.01, s)
    want = G.fast_guided_filter(guide, src, r, 0.01, s)
    assert np.array_equal(got, want), "%d of %d values differ, max |diff| %g" % (
        int((got != want).sum()), got.size, float(np.abs(got.astype(np.float64) - want).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,s,r,channels", [(48, 64, 4, 8, 3), (240, 322, 8, 108, 1), (61, 99, 8, 80, 4)])
def test_device_filter_all_zero_guide_and_other_eps(engine, rows, cols, s, r, channels):
    _, bgr = range_scene(rows, cols, 9)
    src = _src(bgr, channels, 2)
    zero = np.zeros((rows, cols), np.float32)
    assert np.array_equal(_run_filter(engine, zero, src, channels, r, 0.01, s), G.fast_guided_filter(zero, src, r, 0.01, s))
    guide = smooth_guide(rows, cols)
    for eps, scale in ((1e-6, 1.0), (0.5, 0.75)):
        assert np.array_equal(_run_filter(engine, guide, src, channels, r, eps, s, scale),
                              G.fast_guided_filter(guide, src, r, eps, s, scale))


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_device_filter_in_place_and_unaligned(engine, channels):
    """dst == src, and pointers that start 4 bytes into an allocation (the vector path must not be taken)."""
    import torch
    rows, cols, r, eps, s = 61, 99, 22, 0.01, 4
    guide, bgr = range_scene(rows, cols, 17)
    src = _src(bgr, channels, 4)
    want = G.fast_guided_filter(guide, src, r, eps, s)
    d_g, d_p = _dev(guide), _dev(src)
    engine.fast_guided_filter(d_g.data_ptr(), d_p.data_ptr(), rows, cols, channels, r, eps, s, 1.0, d_p.data_ptr())
    engine.synchronize()
    assert np.array_equal(d_p.cpu().numpy(), want)
    n = rows * cols
    buf_g = torch.zeros(n + 1, device="cuda")
    buf_p = torch.zeros(n * channels + 1, device="cuda")
    buf_o = torch.zeros(n * channels + 2, device="cuda")
    buf_g[1:] = _dev(guide).reshape(-1)
    buf_p[1:] = _dev(src).reshape(-1)
    engine.fast_guided_filter(buf_g[1:].data_ptr(), buf_p[1:].data_ptr(), rows, cols, channels, r, eps, s, 1.0,
                              buf_o[1:].data_ptr())
    engine.synchronize()
    out = buf_o.cpu().numpy()
    assert np.array_equal(out[1:-1].reshape(src.shape), want) and out[0] == 0 and out[-1] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(61, 99), (240, 322), (720, 1280)])
def test_device_illuminant_equals_twice_the_definition(engine, rows, cols):
    import torch
    rng_map, bgr = range_scene(rows, cols, cols)
    r, eps, s = G.reference_parameters(cols)
    d_r, d_b = _dev(rng_map), _dev(bgr)
    d_il, d_f = torch.empty_like(d_b), torch.empty_like(d_b)
    engine.estimate_illuminant_range_guided(d_b.data_ptr(), d_r.data_ptr(), rows, cols, r, eps, s, d_il.data_ptr())
    engine.fast_guided_filter(d_r.data_ptr(), d_b.data_ptr(), rows, cols, 3, r, eps, s, 2.0, d_f.data_ptr())
    engine.synchronize()
    il = d_il.cpu().numpy()
    assert np.array_equal(il, np.float32(2) * G.fast_guided_filter(rng_map, bgr, r, eps, s))
    assert np.array_equal(il, G.estimate_illuminant_range_guided(bgr, rng_map, r, eps, s))
    assert torch.equal(d_il, d_f)


def beta_grid(range_map, num_px):
    """The sample positions of EstimateBeta (attenuation.cpp:43-56) before its shuffle: a uniform grid that skips a
    border of 5 pixels, x outer / y inner, kept where range > 1e-3; the first num_px of them."""
    rows, cols = range_map.shape
    per_row = int(np.sqrt(4 * num_px))
    stride_x, stride_y = (cols - 10) // per_row, (rows - 10) // per_row
    pts = [(x, y) for x in range(5, cols - 5, stride_x) for y in range(5, rows - 5, stride_y) if range_map[y, x] > 1e-3]
    return np.array(pts[:num_px], np.int32).reshape(-1, 2)


@pytest.mark.gpu
def test_gather_pixels(pm, engine):
    rows, cols = 240, 322
    rng_map, bgr = range_scene(rows, cols, 21)
    d_r, d_b = _dev(rng_map), _dev(bgr)
    xy = beta_grid(rng_map, 256)
    assert xy.shape == (256, 2)
    for pts in (xy, xy[:1], xy[:0]):
        n = len(pts)
        got3 = engine.gather_pixels(d_b.data_ptr(), rows, cols, 3, xy=pts)
        got1 = engine.gather_pixels(d_r.data_ptr(), rows, cols, 1, xy=pts)
        assert got3.shape == (n, 3) and np.array_equal(got3, bgr[pts[:, 1], pts[:, 0]])
        assert got1.shape == (n, 1) and np.array_equal(got1[:, 0], rng_map[pts[:, 1], pts[:, 0]])
        d_xy = _dev(pts.reshape(-1)) if n else _dev(np.zeros(2, np.int32))
        assert np.array_equal(engine.gather_pixels(d_b.data_ptr(), rows, cols, 3, d_xy=d_xy.data_ptr(), n=n), got3)
        assert np.array_equal(engine.gather_pixels(d_r.data_ptr(), rows, cols, 1, d_xy=d_xy.data_ptr(), n=n), got1)
    # a coordinate outside the image: refused from the host list and from the device list; the stream stays usable
    for bad in ((cols, 3), (4, rows), (-1, 0), (0, -1)):
        pts = xy[:5].copy()
        pts[2] = bad
        with pytest.raises(pm.PmError) as err:
            engine.gather_pixels(d_b.data_ptr(), rows, cols, 3, xy=pts)
        assert err.value.status == pm.PM_ERR_INVALID_ARG
        d_xy = _dev(pts.reshape(-1))
        with pytest.raises(pm.PmError) as err:
            engine.gather_pixels(d_b.data_ptr(), rows, cols, 3, d_xy=d_xy.data_ptr(), n=5)
        assert err.value.status == pm.PM_ERR_INVALID_ARG
        assert np.array_equal(engine.gather_pixels(d_b.data_ptr(), rows, cols, 3, xy=xy[:5]), bgr[xy[:5, 1], xy[:5, 0]])
    with pytest.raises(pm.PmError) as err:  # both lists, or none
        engine.gather_pixels(d_b.data_ptr(), rows, cols, 3, xy=xy, d_xy=d_b.data_ptr())
    assert err.value.status == pm.PM_ERR_INVALID_ARG
    with pytest.raises(pm.PmError) as err:
        engine.gather_pixels(d_b.data_ptr(), rows, cols, 3, n=4)
    assert err.value.status == pm.PM_ERR_INVALID_ARG
    with pytest.raises(pm.PmError) as err:
        engine.gather_pixels(d_b.data_ptr(), rows, cols, 5, xy=xy)
    assert err.value.status == pm.PM_ERR_INVALID_ARG


@pytest.mark.gpu
def test_argument_errors_leave_the_handle_usable(pm, engine):
    import torch
    rows, cols = 48, 64
    guide, bgr = range_scene(rows, cols, 2)
    d_g, d_p = _dev(guide), _dev(bgr)
    d_o = torch.empty_like(d_p)
    g, p, o = d_g.data_ptr(), d_p.data_ptr(), d_o.data_ptr()
    ok = dict(d_guide=g, d_src=p, rows=rows, cols=cols, channels=3, r=8, eps=0.01, s=4, scale=1.0, d_dst=o)
    bad = [dict(d_guide=None), dict(d_src=None), dict(d_dst=None), dict(s=0), dict(s=-2), dict(r=-1), dict(channels=0),
           dict(channels=5), dict(eps=-0.01), dict(eps=float("nan")), dict(eps=float("inf")), dict(s=49), dict(s=65),
           dict(rows=0), dict(cols=0)]
    want = G.fast_guided_filter(guide, bgr, 8, 0.01, 4)
    for change in bad:
        kw = dict(ok, **change)
        with pytest.raises(pm.PmError) as err:
            engine.fast_guided_filter(**kw)
        assert err.value.status == pm.PM_ERR_INVALID_ARG, change
        engine.fast_guided_filter(**ok)
        engine.synchronize()
        assert np.array_equal(d_o.cpu().numpy(), want), change
    for kw in (dict(d_bgr=None, d_range=g), dict(d_bgr=p, d_range=None), dict(d_bgr=p, d_range=g, d_illuminant=None),
               dict(d_bgr=p, d_range=g, s=0), dict(d_bgr=p, d_range=g, r=-2), dict(d_bgr=p, d_range=g, eps=-1.0)):
        full = dict(dict(rows=rows, cols=cols, r=8, eps=0.01, s=4, d_illuminant=o), **kw)
        with pytest.raises(pm.PmError) as err:
            engine.estimate_illuminant_range_guided(**full)
        assert err.value.status == pm.PM_ERR_INVALID_ARG, kw
    engine.estimate_illuminant_range_guided(p, g, rows, cols, 8, 0.01, 4, o)
    engine.synchronize()
    assert np.array_equal(d_o.cpu().numpy(), np.float32(2) * want)


@pytest.mark.gpu
def test_enhance_chain_with_every_image_on_the_device(pm, oracle, synth):
    """Match() -> range -> RemoveBackscatter -> range-guided illuminant -> samples for the fit -> CorrectAttenuation on
    the handle's stream; only the samples cross to the host.  The guided filter is held bit for bit given the same D:
    D carries the expf tolerance of the existing stages, so the device's D is downloaded once for the check."""
    import torch
    rows, cols = 96, 160
    p = synth.make_pair(3, rows, cols)
    bgr = np.random.default_rng(1).uniform(0, 1, (rows, cols, 3)).astype(np.float32)
    r, eps, s = G.reference_parameters(cols)
    with pm.Engine(pm.default_params(0, patch=5, patchmatch_iters=2), max_rows=rows, max_cols=cols) as e:
        L, R = _dev(p["left"]), _dev(p["right"])
        SL, SR = _dev(p["seed_l"]), _dev(p["seed_r"])
        DL, DR = torch.empty_like(SL), torch.empty_like(SR)
        d_bgr = _dev(bgr)
        d_range = torch.empty((rows, cols), device="cuda")
        d_D, d_il, d_out = torch.empty_like(d_bgr), torch.empty_like(d_bgr), torch.empty_like(d_bgr)
        e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), DL.data_ptr(), DR.data_ptr())
        e.disp_to_range(DL.data_ptr(), rows, cols, 400.0, 0.1, d_range.data_ptr())
        e.remove_backscatter(d_bgr.data_ptr(), d_range.data_ptr(), rows, cols, B0, BETA_B0, d_D.data_ptr())
        e.estimate_illuminant_range_guided(d_D.data_ptr(), d_range.data_ptr(), rows, cols, r, eps, s, d_il.data_ptr())
        el, _ = oracle.match(oracle.default_params(0, patch=5, n_iters=2, nthreads=8), p["left"], p["right"], p["seed_l"],
                             p["seed_r"])
        want_range = O.disp_to_range(el, 400.0, 0.1)
        xy = beta_grid(want_range, 64)  # positions depend on the range map alone, which is exact
        assert len(xy) > 16
        got_range = e.gather_pixels(d_range.data_ptr(), rows, cols, 1, xy=xy)
        got_il = e.gather_pixels(d_il.data_ptr(), rows, cols, 3, xy=xy)
        e.correct_attenuation(d_D.data_ptr(), d_range.data_ptr(), rows, cols, X0, d_out.data_ptr())  # X: the caller's fit
        e.synchronize()
        dev_range, dev_D, dev_il, dev_out = (t.cpu().numpy() for t in (d_range, d_D, d_il, d_out))
    assert np.array_equal(dev_range, want_range)
    want_D = O.remove_backscatter(bgr, want_range, B0, BETA_B0)
    np.testing.assert_allclose(dev_D, want_D, rtol=RTOL, atol=ATOL)
    assert np.array_equal(dev_il, G.estimate_illuminant_range_guided(dev_D, dev_range, r, eps, s))
    assert np.array_equal(got_range[:, 0], want_range[xy[:, 1], xy[:, 0]])
    assert np.array_equal(got_il, dev_il[xy[:, 1], xy[:, 0]])
    np.testing.assert_allclose(dev_out, O.correct_attenuation(want_D, want_range, X0), rtol=RTOL, atol=ATOL)


# ---- 9. the C++ mirror ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def guided_exe(tmp_path_factory):
    return build_caller(tmp_path_factory.mktemp("cppguided") / "guided_main", "guided_main.cpp")


def test_guided_mirror_builds_with_gxx(guided_exe):
    assert os.path.isfile(guided_exe)


@pytest.mark.gpu
def test_guided_mirror_matches_the_fixture(guided_exe, tmp_path):
    f = np.load(FIXTURE)
    rows, cols = f["guide"].shape
    f["guide"].tofile(os.path.join(tmp_path, "range.f32"))
    f["src"].tofile(os.path.join(tmp_path, "bgr.f32"))
    res = subprocess.run([guided_exe, str(tmp_path), str(rows), str(cols), str(int(f["r"])), repr(float(f["eps"])),
                          str(int(f["s"]))], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    load = lambda name, shape: np.fromfile(os.path.join(tmp_path, name), np.float32).reshape(shape)
    assert np.array_equal(load("il.f32", (rows, cols, 3)), np.float32(2) * f["output"])
    assert np.array_equal(load("lsac.f32", (rows, cols, 3)), f["output"])
    assert np.array_equal(load("gray.f32", (rows, cols)), f["output"][:, :, 0])
