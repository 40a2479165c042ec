"""Edges of the stereo-ready enhancement (pm_stereo_ready / pm_normalize / pm_gaussian_blur / pm_match_bgr_device,
include/pm/imaging.h) that tests/test_enhance.py's smooth colour-cast images never reach: gray images delivered as BGR
(the second value stretch then has a NEGATIVE or -0.0 minimum), black regions (zero divisors, a first minimum of exactly
0), constant images (vmax == vmin: NaN), negative input to pm_normalize, the tile edges of the separable Gaussian, and
the fused path pm_match_bgr_device against the CPU rather than against pm_stereo_ready (the same device code).

Oracle: oracle/pm_enhance_oracle.c, bit for bit (NaN at the same positions)."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ocean-perception_amd", "csrc")


def gray_bgr(rows, cols, seed):
    """A monochrome camera that delivers 3-channel frames: b == g == r, saturation 0."""
    rng = np.random.default_rng(seed)
    return np.repeat(rng.integers(0, 256, (rows, cols, 1), dtype=np.uint8), 3, -1)


def cast_3b_to_3f(bgr8):
    return bgr8.astype(np.float32) * np.float32(1.0 / 255.0)


def second_stage_minimum(bgr8):
    """The minimum that the SECOND Normalize of the stereo-ready chain stretches by (oracle)."""
    j1 = O.normalize_color_illuminant(cast_3b_to_3f(bgr8))
    return O.value_minmax_eighth(j1.max(-1))[0]


def same(a, b):
    """Bit-for-bit as values: equal where ordered, NaN exactly where the other side has NaN."""
    return np.array_equal(a, b, equal_nan=True)


# (rows, cols, seed): 64x96 has 96 cells of the 1/8 image (one block of the reduction), 136x264 has 17 x 33 = 561 (three
# blocks).  Seeds chosen so that the oracle's second-stage minimum is negative (about half of all seeds are).
GRAY_NEGATIVE = [(64, 96, 1), (64, 96, 9), (136, 264, 8), (136, 264, 3)]
# synth.make_pair indices at 96x160 whose gray-in-BGR images have the property (both images / neither image)
PAIR_NEGATIVE, PAIR_POSITIVE, PAIR_CAST = 29, 20, 28
PAIR_ROWS, PAIR_COLS = 96, 160


def pair_bgr(synth, index, cast=None):
    p = synth.make_pair(index, PAIR_ROWS, PAIR_COLS)
    if cast is None:
        return p, np.repeat(p["left"][..., None], 3, -1), np.repeat(p["right"][..., None], 3, -1)
    c = np.asarray(cast, np.float32)
    return (p, np.clip(p["left"][..., None].astype(np.float32) * c, 0, 255).astype(np.uint8),
            np.clip(p["right"][..., None].astype(np.float32) * c, 0, 255).astype(np.uint8))


# ---- CPU: the fixtures have the property the GPU tests are about ------------------------------------------------------
def test_gray_fixtures_have_a_negative_second_stage_minimum(synth):
    for rows, cols, seed in GRAY_NEGATIVE:
        lo = second_stage_minimum(gray_bgr(rows, cols, seed))
        assert np.signbit(lo), (rows, cols, seed, lo)
    for img in pair_bgr(synth, PAIR_NEGATIVE)[1:]:
        assert np.signbit(second_stage_minimum(img))
    for img in pair_bgr(synth, PAIR_POSITIVE)[1:] + pair_bgr(synth, PAIR_CAST, (0.9, 0.7, 0.35))[1:]:
        lo = second_stage_minimum(img)
        assert lo > 0 and not np.signbit(lo)
    # a colour cast (s > 0) keeps it positive: why tests/test_enhance.py never met the case
    from test_enhance import color_image
    assert second_stage_minimum(color_image(64, 96, 64 * 3 + 96)) > 0


def black_half(rows, cols, seed):
    img = gray_bgr(rows, cols, seed)
    img[:, :cols // 2] = 0
    return img


def black_rectangle(rows, cols, seed):
    from test_enhance import color_image
    img = color_image(rows, cols, seed)
    img[rows // 9:rows - rows // 9, cols // 4:cols - cols // 5] = 0  # larger than the Gaussian in both directions
    return img


def test_black_regions_give_zero_divisors_and_a_zero_first_minimum():
    for img in (black_half(64, 96, 3), black_rectangle(72, 120, 4)):
        f = cast_3b_to_3f(img)
        third = img.shape[1] // 3
        ksize = third + (1 - third % 2)
        blur = O.gaussian_blur(f, ksize, float(np.float32(ksize) / np.float32(4.0)))
        d = blur * np.float32(2.0)
        assert (d == 0).any(), "illuminant_div's d != 0 branch"
        q = np.where(d != 0, f / np.where(d != 0, d, np.float32(1)), np.float32(0)).astype(np.float32)
        lo, hi = O.value_minmax_eighth(q.max(-1))
        assert lo == 0.0 and hi > 0.0
        J, gray = O.stereo_ready(img)
        assert not np.isnan(J).any() and gray.max() == 255


def test_oracle_constant_image_is_nan_with_zero_bytes():
    """vmax == vmin: alpha = 1 / 0, beta = -vmin / 0; the second stage sees only NaN and keeps FLT_MAX / -FLT_MAX."""
    for c in (0, 77, 255):
        J, gray = O.stereo_ready(np.full((16, 24, 3), c, np.uint8))
        assert np.isnan(J).all() and not gray.any()
    lo, hi = O.value_minmax_eighth(np.full((16, 24), np.nan, np.float32))
    assert lo == float(np.finfo(np.float32).max) and hi == -lo


# ---- device --------------------------------------------------------------------------------------------------------
def _dev(t, a):
    return t.from_numpy(np.ascontiguousarray(a)).cuda()


def _stereo_ready(torch, e, bgr8):
    rows, cols = bgr8.shape[:2]
    d_b = _dev(torch, bgr8)
    d_J = torch.empty((rows, cols, 3), device="cuda")
    d_g = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
    e.stereo_ready(d_b.data_ptr(), rows, cols, d_J.data_ptr(), d_g.data_ptr())
    e.synchronize()
    return d_J.cpu().numpy(), d_g.cpu().numpy()


def _normalize(torch, e, f):
    rows, cols = f.shape[:2]
    d_f = _dev(torch, f)
    d_n = torch.empty_like(d_f)
    e.normalize(d_f.data_ptr(), rows, cols, d_n.data_ptr())
    e.synchronize()
    return d_n.cpu().numpy()


def _check_stereo_ready(torch, e, bgr8, what):
    J, gray = _stereo_ready(torch, e, bgr8)
    want_J, want_gray = O.stereo_ready(bgr8)
    assert same(J, want_J), f"{what}: J, {int((~np.isclose(J, want_J, rtol=0, atol=0, equal_nan=True)).sum())} differ"
    assert np.array_equal(gray, want_gray), f"{what}: 8-bit gray, {int((gray != want_gray).sum())} differ"
    return want_J


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,seed", GRAY_NEGATIVE)
def test_device_gray_in_bgr_is_bit_exact(pm, rows, cols, seed):
    """Fails on a reduction that orders the value bits as unsigned integers: at 64x96 the minimum word stays FLT_MAX and
    the whole image collapses, at 136x264 another block's positive minimum takes its place."""
    import torch
    bgr8 = gray_bgr(rows, cols, seed)
    with pm.Engine(pm.default_params(0, patch=5), max_rows=16, max_cols=16) as e:
        _check_stereo_ready(torch, e, bgr8, "gray in BGR")
        j1 = O.normalize_color_illuminant(cast_3b_to_3f(bgr8))  # = O.normalize(q): its stretched minimum sits at -0
        assert np.array_equal(_normalize(torch, e, j1), O.normalize(j1)), "pm_normalize of a stretched gray image"


@pytest.mark.gpu
def test_device_zero_divisors_and_zero_minimum(pm):
    import torch
    with pm.Engine(pm.default_params(0, patch=5), max_rows=16, max_cols=16) as e:
        J = _check_stereo_ready(torch, e, black_half(64, 96, 3), "left half black")
        assert not np.isnan(J).any()
        _check_stereo_ready(torch, e, black_rectangle(72, 120, 4), "black rectangle")


@pytest.mark.gpu
def test_device_constant_images_are_nan_like_the_oracle(pm):
    """include/pm/imaging.h: a constant image gives NaN in every value of J and 0 in every gray byte."""
    import torch
    with pm.Engine(pm.default_params(0, patch=5), max_rows=16, max_cols=16) as e:
        for c in (0, 77, 255):
            J, gray = _stereo_ready(torch, e, np.full((16, 24, 3), c, np.uint8))
            assert np.isnan(J).all() and not gray.any(), c
            _check_stereo_ready(torch, e, np.full((40, 64, 3), c, np.uint8), f"constant {c}")
        f = np.full((16, 24, 3), 0.25, np.float32)
        assert same(_normalize(torch, e, f), O.normalize(f)) and np.isnan(O.normalize(f)).all()
        # one channel differs: s > 0, still vmax == vmin
        f[..., 1] = 0.125
        assert same(_normalize(torch, e, f), O.normalize(f))


@pytest.mark.gpu
def test_device_normalize_takes_negative_input(pm):
    """pm_normalize is a public entry point: some negative channels, all-negative pixels, an all-negative image (the
    maximum of the 1/8 image is then negative as well: it must not start at 0)."""
    import torch
    rng = np.random.default_rng(11)
    rows, cols = 50, 77
    some = rng.uniform(-0.3, 1.0, (rows, cols, 3)).astype(np.float32)
    pixels = rng.uniform(0.05, 1.0, (rows, cols, 3)).astype(np.float32)
    pixels[rng.random((rows, cols)) < 0.3] *= np.float32(-1.0)
    pixels[8:24, 16:40] = -np.abs(pixels[8:24, 16:40])  # whole cells of the 1/8 image negative
    allneg = rng.uniform(-1.0, -0.05, (136, 264, 3)).astype(np.float32)
    with pm.Engine(pm.default_params(0, patch=5), max_rows=16, max_cols=16) as e:
        for name, f in (("some negative channels", some), ("all-negative pixels", pixels), ("all negative", allneg)):
            lo, hi = O.value_minmax_eighth(f.max(-1))
            assert (f < 0).any() and (lo < 0 or name == "some negative channels")
            assert (hi < 0) == (name == "all negative")
            want = O.normalize(f)
            assert not np.isnan(want).any()
            assert np.array_equal(_normalize(torch, e, f), want), name


def _int_constant(name, header="pm_enhance.hpp"):
    src = open(os.path.join(CSRC, header)).read()
    m = re.search(r"constexpr int %s = ([^;]+);" % name, src)
    assert m, name
    expr = m.group(1)
    for other in re.findall(r"k[A-Z]\w+", expr):
        expr = expr.replace(other, str(_int_constant(other, header)))
    return int(eval(expr, {"__builtins__": {}}))


def column_tile_rows(ksize):
    """T of run_gaussian_batch (pm_imaging.hip): the widest of W = 32, 16, 8 whose tile of T = (256 / (W / 2)) * 4 output
    rows fits 48 KB of LDS, ((T + 2c + 3) * (W + 2) + c + 1) floats."""
    src = open(os.path.join(CSRC, "pm_imaging.hip")).read()
    assert "for (int w : {32, 16, 8})" in src and "const int t = (256 / (w / 2)) * 4;" in src
    assert "lds_of(w, t) <= 48 * 1024" in src
    assert "sizeof(float) * ((size_t)(t + 2 * c + 3) * (w + 2) + c + 1)" in src
    c = ksize // 2
    for w in (32, 16, 8):
        t = (256 // (w // 2)) * 4
        if 4 * ((t + 2 * c + 3) * (w + 2) + c + 1) <= 48 * 1024:
            return t
    raise AssertionError(ksize)


def test_tile_constants_read_from_the_source():
    assert _int_constant("kBlurRowPx") == 4 * _int_constant("kBlurRowThreads")
    # the three column tiles all occur among the kernel sizes the tile-edge test uses
    assert [column_tile_rows(k) for k in (9, 291, 293, 537, 539)] == [64, 64, 128, 128, 256]


def _blur_cases():
    px = _int_constant("kBlurRowPx")
    cases = []
    for ch in (1, 3):
        t = column_tile_rows(9)
        for cols in (px - 1, px, px + 1):
            for rows in (t - 1, t, t + 1):
                cases.append((rows, cols, ch, 9))
    for ksize, cols, ch in ((293, 40, 1), (539, 24, 3)):  # the narrower column tiles W = 16 and W = 8
        t = column_tile_rows(ksize)
        cases += [(rows, cols, ch, ksize) for rows in (t - 1, t, t + 1)]
    cases += [(13, 21, 1, 1), (13, 21, 3, 1), (70, px + 1, 3, 1)]  # one tap
    cases += [(13, 21, 1, 3), (9, 10, 3, 3), (70, px + 1, 3, 3)]   # fewer taps than the row pass's register block
    cases += [(20, 30, 3, 61), (8, 8, 1, 17)]                      # ksize larger than both rows and cols
    return cases


@pytest.mark.gpu
def test_device_gaussian_tile_edges(pm):
    """cols one below / at / one above the row tile, rows one below / at / one above the column tile that the launcher
    picks for the kernel size (all three tile widths), 1 and 3 taps, and kernels larger than the image."""
    import torch
    rng = np.random.default_rng(5)
    with pm.Engine(pm.default_params(0, patch=5), max_rows=16, max_cols=16) as e:
        for rows, cols, ch, ksize in _blur_cases():
            img = rng.uniform(0, 1, (rows, cols, ch) if ch > 1 else (rows, cols)).astype(np.float32)
            sigma = max(ksize, 3) / 4.0
            d_in = _dev(torch, img)
            d_out = torch.full_like(d_in, -1.0)
            e.gaussian_blur(d_in.data_ptr(), rows, cols, ch, ksize, sigma, d_out.data_ptr())
            e.synchronize()
            want = O.gaussian_blur(img, ksize, sigma)
            got = d_out.cpu().numpy()
            assert np.array_equal(got, want), (rows, cols, ch, ksize, int((got != want).sum()))
            if ksize == 1:
                assert np.array_equal(want, img)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(8, 8), (9, 11), (16, 8), (8, 16)])
def test_device_smallest_images_through_stereo_ready(pm, rows, cols):
    """8x8 is the smallest legal image: one cell of the 1/8 image, a Gaussian of NextOddInt(cols / 3) = 3 taps (5 from 12
    columns on).  One cell means vmax == vmin in the FIRST stretch: NaN like a constant image; 16x8 and 8x16 have two."""
    import torch
    from test_enhance import color_image
    with pm.Engine(pm.default_params(0, patch=5), max_rows=16, max_cols=16) as e:
        _check_stereo_ready(torch, e, color_image(rows, cols, rows + cols), "smallest")
        _check_stereo_ready(torch, e, gray_bgr(rows, cols, rows + cols), "smallest gray")
        # the quotient image in front of the stretch, which is not NaN: I / (2 blur) through the float entry points
        f = cast_3b_to_3f(color_image(rows, cols, 3))
        third = cols // 3
        ksize = third + (1 - third % 2)
        sigma = float(np.float32(ksize) / np.float32(4.0))
        d_in = _dev(torch, f)
        d_out = torch.empty_like(d_in)
        e.gaussian_blur(d_in.data_ptr(), rows, cols, 3, ksize, sigma, d_out.data_ptr())
        e.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), O.gaussian_blur(f, ksize, sigma))


# ---- the fused path against the CPU ---------------------------------------------------------------------------------
_fused_cache = {}


def _fused_batches(synth):
    """Two batches of two pairs; in each, one pair's images have the negative second-stage minimum and the other's not."""
    if "b" not in _fused_cache:
        neg, pos = pair_bgr(synth, PAIR_NEGATIVE), pair_bgr(synth, PAIR_POSITIVE)
        cast = pair_bgr(synth, PAIR_CAST, (0.9, 0.7, 0.35))
        _fused_cache["b"] = {"gray_gray": [neg, pos], "cast_gray": [cast, neg]}
        _fused_cache["g"] = {}
    return _fused_cache["b"]


def _oracle_grays(synth, name):
    batch = _fused_batches(synth)[name]
    if name not in _fused_cache["g"]:
        _fused_cache["g"][name] = [(O.stereo_ready(bl)[1], O.stereo_ready(br)[1]) for _, bl, br in batch]
    return _fused_cache["g"][name]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["gray_gray", "cast_gray"])
@pytest.mark.parametrize("mode", ["scalar", "planes_f16"])
def test_fused_bgr_match_against_the_cpu(pm, oracle, synth, mode, batch):
    """pm_match_bgr_device vs oracle.match on O.stereo_ready grays (tests/test_enhance.py compares it with
    pm_stereo_ready only, the same device code).  n = 2: image y's words live at mm + 4 y, and the two pairs of a batch
    differ in the sign of their second-stage minimum, so cross-talk between the words shows."""
    import torch
    rows, cols, n = PAIR_ROWS, PAIR_COLS, 2
    pairs = _fused_batches(synth)[batch]
    grays = _oracle_grays(synth, batch)
    if mode == "scalar":
        prm = pm.default_params(0, patch=5, patchmatch_iters=2)
    else:
        prm = pm.default_params(0, patch=7, patchmatch_iters=2, mode=pm.PM_MODE_PLANES, max_disp=48,
                                state_dtype=pm.PM_STATE_F16)
    dev = torch.device("cuda")
    BL = torch.from_numpy(np.stack([bl for _, bl, _ in pairs])).to(dev).contiguous()
    BR = torch.from_numpy(np.stack([br for _, _, br in pairs])).to(dev).contiguous()
    DL = torch.empty((n, rows, cols), dtype=torch.float32, device=dev)
    DR = torch.empty_like(DL)
    SL = SR = None
    if mode == "scalar":
        SL = torch.from_numpy(np.stack([p["seed_l"] for p, _, _ in pairs])).to(dev).contiguous()
        SR = torch.from_numpy(np.stack([p["seed_r"] for p, _, _ in pairs])).to(dev).contiguous()
    with pm.Engine(prm, max_rows=rows, max_cols=cols, max_batch=n) as e:
        e.match_bgr_device(n, BL.data_ptr(), BR.data_ptr(), rows, cols, SL.data_ptr() if SL is not None else None,
                           SR.data_ptr() if SR is not None else None, DL.data_ptr(), DR.data_ptr())
        e.synchronize()
    got_l, got_r = DL.cpu().numpy(), DR.cpu().numpy()
    for i, ((p, _, _), (gl, gr)) in enumerate(zip(pairs, grays)):
        if mode == "scalar":
            el, er = oracle.match(oracle.default_params(0, patch=5, n_iters=2, nthreads=8), gl, gr, p["seed_l"],
                                  p["seed_r"])
        else:
            el, er = oracle.planes_match(oracle.planes_params(**oracle.planes_kwargs_of(prm, nthreads=8)), gl, gr)
        assert (el > 0).mean() > 0.2
        assert np.array_equal(got_l[i], el), f"pair {i} left: {int((got_l[i] != el).sum())} pixels differ"
        assert np.array_equal(got_r[i], er), f"pair {i} right: {int((got_r[i] != er).sum())} pixels differ"
