"""The CPU oracle and the HIP engine against the reference's OWN compiled code.

oracle/_ref/libpm_ref.so is the reference's stereo_matching/patchmatch.cpp (AddNoise, both PropagateNeighbors, Propagate,
RemoveBackground) and the cost functor and ComputeGradient of its test/stereo_matching/patchmatch_test.cpp, compiled from
the reference tree with g++ -O3 -ffp-contract=off against this project's OpenCV stand-in (oracle/ref/; tests/ref_lib.py
loads it).  Everything that is the reference author's text is therefore executed here, not restated: the float loop
counters, the skip rule, the double-promoted clamp with its integer division, the >= acceptance test, the strict first
minimum, the write of the clamped d0, the (patch_height, patch_width) order, the functor's trip through 8-bit gradient
patches, cost_no_disp / win_by_factor.  What stays restated is OpenCV underneath (the stand-in), checked in section (a).

  (a) the stand-in's primitives against scipy / numpy / hand-computed values, then against the oracle's bit for bit
  (b) the oracle against the compiled reference, function by function, TOLERANCE 0
  (c) the same inputs through the HIP engine (PM_SEM_CPU), against the compiled reference directly, tolerance 0 (-m gpu)
  (d) the reference built with its own flags (contraction allowed) against its uncontracted build: the stated tolerance
  (e) fixtures recorded from the compiled reference (tests/golden/ref_*.npz): these never skip

Tolerance 0 in (b), (c), (e) is derived, not measured: with contraction off both sides are the same sequence of IEEE-754
binary32 / binary64 operations.  Tests that need the library skip, naming the recipe, where oracle/_ref/ was not built.
"""
import os

import numpy as np
import pytest

import ref_lib
from conftest import GOLDEN, ROOT, assert_same
from ref_inputs import (PROPAGATE_CASES, PROPAGATE_IDS, RECIPE_SCHEDULE, WINDOWS, contraction_counts, farmsim_inputs,
                        oracle_recipe, synthetic_recipe_inputs, tolerance_inputs)

ENGINES = [1, 2, 5]  # as tests/test_gpu_parity.py: PM_ENGINE_SERIAL, _WAVE, _RUNBLK2
# What the engine can be given of the cases of (b).  The C ABI refuses images below 8 x 8 (check_size, pm_engine.hip), so
# of the edge sizes it sees `rows == ph` for 11x11 only, `rows == ph + 1` for 7x3 and 11x11, `cols == pw + 1` for 11x11;
# the smaller ones are held on the CPU side, oracle against reference.  Maps with negative values: pm_remove_background
# takes them (d0 is clamped, as in the reference); pm_propagate refuses them (include/pm/patchmatch.h) -- the reference
# tries a neighbour's negative disparity with the window beyond the right border, which the kernels do not implement.
ENGINE_CASES = [c for c in PROPAGATE_CASES if min(c[1].shape) >= 8]
PROFILE = os.path.join(ROOT, "profiles", "ref_contract_tolerance.txt")


@pytest.fixture(scope="module")
def ref():
    return ref_lib.load_or_skip()


@pytest.fixture(scope="module")
def ref_contracted():
    return ref_lib.load_or_skip(ref_lib.CONTRACTED_PATH)


# ---- (a) the stand-in's primitives ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ndi():
    return pytest.importorskip("scipy.ndimage")


@pytest.mark.parametrize("shape", [(5, 7), (16, 16), (33, 20), (2, 9), (64, 48)])
def test_standin_sobel_equals_scipy_sobel_with_mirror_border(ref, ndi, shape):
    rng = np.random.default_rng(shape[0] * 131 + shape[1])
    im = rng.integers(0, 256, shape, dtype=np.uint8)
    f = im.astype(np.float64)
    sx = ndi.sobel(f, axis=1, mode="mirror")
    sy = ndi.sobel(f, axis=0, mode="mirror")
    assert np.array_equal(ref.sobel(im, 1, 0), sx.astype(np.float32))
    assert np.array_equal(ref.sobel(im, 0, 1), sy.astype(np.float32))
    want = np.sqrt((sx * sx + sy * sy).astype(np.float32))
    assert np.array_equal(ref.compute_gradient(im), want.astype(np.float32))


def _patch_coords(pw, ph, cx, cy):
    ys = cy - (ph - 1) * 0.5 + np.arange(ph)
    xs = cx - (pw - 1) * 0.5 + np.arange(pw)
    return np.meshgrid(ys, xs, indexing="ij")


SUBPIX_CENTRES = [(10.0, 9.0), (10.25, 9.5), (3.7, 2.1), (0.4, 0.2), (30.9, 21.6), (-1.5, 12.0), (33.5, 25.0),
                  (-9.0, -9.0), (16.0, 40.0)]   # the last four: the window leaves the image, partly or wholly


@pytest.mark.parametrize("cx,cy", SUBPIX_CENTRES)
def test_standin_rect_subpix_f32_equals_scipy_bilinear_with_replicated_border(ref, ndi, cx, cy):
    rng = np.random.default_rng(3)
    img = rng.uniform(0, 1400, (24, 33)).astype(np.float32)
    for pw, ph in ((3, 3), (7, 5), (11, 11)):
        yy, xx = _patch_coords(pw, ph, cx, cy)
        want = ndi.map_coordinates(img.astype(np.float64), [yy, xx], order=1, mode="nearest")
        got = ref.get_rect_subpix(img, pw, ph, cx, cy)
        assert np.allclose(got, want, rtol=1e-4, atol=1e-3), (pw, ph, np.abs(got - want).max())


@pytest.mark.parametrize("cx,cy", SUBPIX_CENTRES)
def test_standin_rect_subpix_u8_is_the_rounded_scipy_bilinear(ref, ndi, cx, cy):
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (24, 33), dtype=np.uint8)
    for pw, ph in ((3, 3), (7, 5), (11, 11)):
        yy, xx = _patch_coords(pw, ph, cx, cy)
        exact = ndi.map_coordinates(img.astype(np.float64), [yy, xx], order=1, mode="nearest")
        got = ref.get_rect_subpix(img, pw, ph, cx, cy).astype(np.float64)
        assert np.abs(got - exact).max() <= 0.5 + 2.0 ** -7
        clear = np.abs((exact - np.floor(exact)) - 0.5) > 2.0 ** -7
        assert np.array_equal(got[clear], np.rint(exact[clear]))


def test_standin_rect_subpix_known_answers(ref):
    src = np.arange(8 * 10, dtype=np.uint8).reshape(8, 10) * 2
    assert np.array_equal(ref.get_rect_subpix(src, 3, 3, 4.0, 3.0), src[2:5, 3:6])      # integer centre: a copy
    assert np.array_equal(ref.get_rect_subpix(src, 3, 1, 4.5, 3.0)[0], src[3, 3:6] + 1)  # half-way, rounded up
    assert ref.get_rect_subpix(src, 1, 1, 4.25, 3.0)[0, 0] == src[3, 4] + 1
    assert np.array_equal(ref.get_rect_subpix(src, 3, 3, 0.0, 0.0), src[np.ix_([0, 0, 1], [0, 0, 1])])
    srcf = src.astype(np.float32)
    p = ref.get_rect_subpix(srcf, 3, 1, 4.25, 3.0)
    assert np.array_equal(p[0], srcf[3, 3:6] * np.float32(0.75) + srcf[3, 4:7] * np.float32(0.25))


def test_standin_rng_first_outputs_by_hand_and_both_saturate_range_values(ref):
    s1 = 123 * 4164903690
    s2 = (s1 & 0xFFFFFFFF) * 4164903690 + (s1 >> 32)
    raw = ref.rng_raw(2, 123)
    assert int(raw[0]) == s1 & 0xFFFFFFFF and int(raw[1]) == s2 & 0xFFFFFFFF
    assert int(ref.rng_raw(1, 0)[0]) == (0xFFFFFFFF * 4164903690) & 0xFFFFFFFF      # seed 0 becomes 2^32 - 1
    # fill: (float)(int)raw * (float)(min(limit, hi - lo) * 2^-32) + (float)((hi + lo) / 2), one rounding per step
    raw = ref.rng_raw(64, 123).astype(np.int32).astype(np.float32)

    def by_hand(lo, hi, limit):
        scale = np.float32(min(limit, hi - lo) * 2.0 ** -32)
        return (raw * scale).astype(np.float32) + np.float32((hi + lo) * 0.5)

    f32max, f64max = float(np.finfo(np.float32).max), float(np.finfo(np.float64).max)
    for lo, hi in ((-32.0, 32.0), (-0.5, 0.5), (0.0, 7.0)):                       # an ordinary range: the flag is idle
        for flag, limit in ((False, f64max), (True, f32max)):
            got = ref.rng_fill(8, 8, lo, hi, flag).ravel()
            assert np.array_equal(got, by_hand(lo, hi, limit)) and got.min() >= lo and got.max() < hi
    lo, hi = -3e38, 3e38                                                          # hi - lo exceeds FLT_MAX: the flag acts
    wide, clamped = ref.rng_fill(8, 8, lo, hi, False).ravel(), ref.rng_fill(8, 8, lo, hi, True).ravel()
    assert np.array_equal(wide, by_hand(lo, hi, f64max)) and np.array_equal(clamped, by_hand(lo, hi, f32max))
    assert not np.array_equal(wide, clamped)


def test_standin_f32_to_u8_saturation(ref):
    """Mat_<uchar>(Mat_<float>): cvRound (ties to even), then the clamp to 0..255."""
    src = np.array([[-0.5, 0.5, 1.5, 254.5, 255.5, 300.0, -3.0, 2.5, 0.49999997, 254.50002, 1441.7]], np.float32)
    assert ref.convert_f32_u8(src).tolist() == [[0, 0, 2, 254, 255, 255, 0, 2, 0, 255, 255]]
    rng = np.random.default_rng(9)
    a = rng.uniform(-50, 400, (37, 41)).astype(np.float32)
    assert np.array_equal(ref.convert_f32_u8(a), np.clip(np.rint(a), 0, 255).astype(np.uint8))


def test_standin_mean(ref):
    rng = np.random.default_rng(10)
    for shape in ((3, 3), (5, 3), (11, 11)):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        assert ref.mean(a) == float(a.sum(dtype=np.int64)) * (1.0 / a.size)        # the reciprocal, not a division
        whole = a.astype(np.float32)                                               # what the functor's 32f mean sees
        assert ref.mean(whole) == ref.mean(a)
        f = rng.uniform(0, 1400, shape).astype(np.float32)
        assert abs(ref.mean(f) - f.astype(np.float64).mean()) <= 1e-6 * 1400


def test_standin_primitives_equal_the_oracles_bit_for_bit(ref, oracle):
    """Two restatements written apart: the stand-in (oracle/ref/cv_standin.cpp) and oracle/pm_oracle.c."""
    rng = np.random.default_rng(11)
    assert np.array_equal(ref.rng_raw(4096, 123), oracle.rng_raw(4096, 123))
    for amount in (32.0, 8.0, 2.0, 0.5, 1.0):
        assert np.array_equal(ref.rng_fill(50, 70, -amount, amount).ravel(), oracle.rng_fill_uniform(3500, -amount, amount))
    src8 = rng.integers(0, 256, (20, 30), dtype=np.uint8)
    srcf = (rng.random((20, 30)) * 1400).astype(np.float32)
    for _ in range(1500):
        pw, ph = int(rng.choice([3, 5, 7, 11])), int(rng.choice([3, 5, 7, 11]))
        x = float(np.float32(rng.uniform(-8, 38)))                                 # in and out of the image
        y = float(np.float32(rng.uniform(-8, 28)))
        if rng.random() < 0.5:
            y = float(int(y))                                                      # integer rows, as on the path
        for src in (src8, srcf):
            a, b = ref.get_rect_subpix(src, pw, ph, x, y), oracle.get_rect_subpix(src, pw, ph, x, y)
            assert np.array_equal(a, b), (pw, ph, x, y, src.dtype)
    for shape in ((2, 9), (33, 20), (64, 48), (7, 2)):
        im = rng.integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(ref.compute_gradient(im), oracle.gradient_magnitude(im))


# ---- (b) the oracle against the compiled reference, tolerance 0 -----------------------------------------------------
@pytest.mark.parametrize("amount", [32.0, 8.0, 2.0, 0.5])
def test_add_noise(ref, oracle, amount):
    rng = np.random.default_rng(12)
    d = rng.uniform(-6.0, 40.0, (45, 70)).astype(np.float32)
    d[rng.random(d.shape) < 0.4] = 0.0                                             # zeros and negative values
    mask = ((d > 0) * 255).astype(np.uint8)
    assert_same(oracle.cpu_add_noise(d, amount, mask), ref.add_noise(d, amount, mask), f"AddNoise {amount}, disp > 0")
    assert_same(oracle.cpu_add_noise(d, amount, None), ref.add_noise(d, amount, None), f"AddNoise {amount}, no mask")
    assert ref.add_noise(d, amount, None).min() >= 0.0


@pytest.mark.parametrize("shape", [(2, 9), (33, 20), (64, 48), (5, 7), (240, 376)])
def test_compute_gradient(ref, oracle, shape):
    rng = np.random.default_rng(shape[0])
    im = rng.integers(0, 256, shape, dtype=np.uint8)
    assert_same(oracle.gradient_magnitude(im), ref.compute_gradient(im), "ComputeGradient")


def functor_cases():
    rng = np.random.default_rng(13)
    cases = []
    for ph, pw in ((3, 3), (5, 3), (5, 5), (11, 11)):
        shape = (ph, pw)
        for _ in range(12):                                                        # plain random patches
            cases.append((rng.integers(0, 256, shape), rng.integers(0, 256, shape), rng.uniform(0, 1442, shape),
                          rng.uniform(0, 1442, shape)))
        for _ in range(8):    # gradients above 255 and on fractional halves: only the 8-bit saturation makes them agree
            g = rng.integers(0, 300, shape) + 0.5
            cases.append((rng.integers(0, 256, shape), rng.integers(0, 256, shape), g, g + rng.integers(-3, 4, shape) * 0.5))
            cases.append((rng.integers(0, 256, shape), rng.integers(0, 256, shape), rng.uniform(250, 262, shape),
                          rng.uniform(200, 1442, shape)))
        base = rng.integers(0, 200, shape)
        for delta in (0, 1, 48, 49, 50, 51, 52):                                   # colour error on both sides of tau_color
            for gdelta in (0.0, 18.0, 19.0, 20.0, 21.0, 22.0, 19.5):               # gradient error around tau_grad
                gbase = rng.integers(0, 200, shape).astype(np.float64)
                cases.append((base, base + delta, gbase, gbase + gdelta))
        one_off = base.copy()                                                      # mean error just off the thresholds
        one_off[0, 0] += 1
        cases.append((base, one_off + 50, base.astype(np.float64), base + 20.0))
        cases.append((one_off, base + 50, base.astype(np.float64), one_off + 20.0))
        cases.append((base, base, base * 1.25, base * 1.25))                       # equal patches
    return [(np.asarray(a, np.uint8), np.asarray(b, np.uint8), np.asarray(c, np.float32), np.asarray(d, np.float32))
            for a, b, c, d in cases]


def test_functor(ref, oracle):
    costs = set()
    for pl, pr, gl, gr in functor_cases():
        ph, pw = pl.shape
        want = np.float32(ref.functor(pl, pr, gl, gr))
        costs.add(float(want))
        assert np.float32(oracle.cpu_functor(pl, pr, gl, gr)) == want, ("cpu_functor", pl.shape)
        # the patches as whole images, the window in their middle, disparity 0: getRectSubPix returns them unchanged
        ims = oracle.ImageSet(pl, pr, gl, gr)
        for literal in (True, False):
            got = np.float32(oracle.cpu_cost(ims, pw, ph, pw // 2, ph // 2, 0.0, literal=literal))
            assert got == want, ("cpu_cost", literal, pl.shape, got, want)
    assert 0.0 in costs and float(np.float32(0.7) * np.float32(50.0) + (np.float32(1) - np.float32(0.7)) * np.float32(20.0)) in costs
    assert len(costs) > 100


@pytest.mark.parametrize("case", PROPAGATE_CASES, ids=PROPAGATE_IDS)
def test_propagate(ref, oracle, case):
    name, l, r, d, ph, pw = case
    want = ref.propagate(l, r, d, ph, pw)
    ims = oracle.ImageSet(l, r)
    for literal in (False, True):
        assert_same(oracle.cpu_propagate(ims, d, ph, pw, pass_mask=15, literal=literal, nthreads=4), want,
                    f"Propagate {name} literal={literal}")
    chain = d
    for mask in (1, 2, 4, 8):                                                      # the order is the reference's
        chain = oracle.cpu_propagate(ims, chain, ph, pw, pass_mask=mask)
    assert_same(chain, want, f"Propagate {name}, pass by pass")


def test_propagate_cases_are_not_vacuous(ref, oracle):
    """The cases do what they claim: the pass order matters on them, the maps change, the edge field meets the >= test
    as an equality and the candidate behind it gets accepted somewhere."""
    by_id = {c[0]: c for c in PROPAGATE_CASES}
    _, l, r, d, ph, pw = by_id["5x5-99x61-truth_noise"]
    want = ref.propagate(l, r, d, ph, pw)
    assert (want != d).mean() > 0.2
    ims = oracle.ImageSet(l, r)
    swapped = d
    for mask in (1, 4, 2, 8):
        swapped = oracle.cpu_propagate(ims, swapped, ph, pw, pass_mask=mask)
    assert not np.array_equal(swapped, want)
    for ph, pw in WINDOWS:
        _, l, r, d, _, _ = by_id[f"{ph}x{pw}-99x61-edge"]
        out = ref.propagate(l, r, d, ph, pw)
        xs = np.arange(d.shape[1], dtype=np.float32)[None, :]
        assert ((out == xs - (pw // 2)) & (out != d))[ph // 2:-(ph // 2), pw // 2 + 1:-(pw // 2)].any(), (ph, pw)
    _, l, r, d, ph, pw = by_id["5x5-constant-fractional"]                          # all ties: nothing moves but the clamp
    out = ref.propagate(l, r, d, ph, pw)
    xs = np.arange(d.shape[1], dtype=np.float32)[None, :]
    inner = np.zeros(d.shape, bool)
    inner[2:-2, 2:-2] = True
    assert np.array_equal(out[inner], np.minimum(d, xs - 2)[inner]) and np.array_equal(out[~inner], d[~inner])


@pytest.mark.parametrize("factor", [1.5, 2.0])
@pytest.mark.parametrize("case", PROPAGATE_CASES, ids=PROPAGATE_IDS)
def test_remove_background(ref, oracle, case, factor):
    name, l, r, d, ph, pw = case
    # 2.0 is the header's default: the reference is called WITHOUT the argument there
    want = ref.remove_background(l, r, d, ph, pw, None if factor == 2.0 else factor)
    ims = oracle.ImageSet(l, r)
    for literal in (False, True):
        assert_same(oracle.cpu_remove_background(ims, d, ph, pw, factor, literal=literal), want,
                    f"RemoveBackground {name} / {factor} literal={literal}")
    prop = ref.propagate(l, r, d, ph, pw)                                          # and on a propagated map
    assert_same(oracle.cpu_remove_background(ims, prop, ph, pw, factor),
                ref.remove_background(l, r, prop, ph, pw, None if factor == 2.0 else factor),
                f"RemoveBackground after Propagate {name} / {factor}")


def test_recipe_farmsim(ref, oracle):
    l, r, seed = farmsim_inputs(oracle)
    want = ref.recipe(l, r, seed)
    assert (want > 0).mean() > 0.3
    for literal in (1, 0):
        assert_same(oracle_recipe(oracle, l, r, seed, literal), want, f"the test's recipe on fsl1 / fsr1, literal={literal}")


def test_recipe_synthetic_96x150(ref, oracle, synth):
    l, r, seed = synthetic_recipe_inputs(synth)
    want = ref.recipe(l, r, seed)
    assert (want > 0).mean() > 0.2
    for literal in (1, 0):
        assert_same(oracle_recipe(oracle, l, r, seed, literal), want, f"the test's recipe on 150x96, literal={literal}")


# ---- (c) the HIP engine against the compiled reference, tolerance 0 ---------------------------------------------------
def _engine(pm, engine, rows, cols, **kw):
    p = pm.default_params(0, patch=3, patchmatch_iters=3, engine=engine, left_right_check=0, **kw)
    return pm.Engine(p, max_rows=rows, max_cols=cols)


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ENGINES)
def test_engine_propagate_and_remove_background_equal_the_compiled_reference(ref, pm, engine):
    """Every case of (b) that the C ABI accepts, on one handle per engine.  A map with a negative value is refused by
    pm_propagate with PM_ERR_INVALID_ARG before anything is launched; RemoveBackground runs on all of them."""
    refused = 0
    with _engine(pm, engine, 64, 104) as e:
        for name, l, r, d, ph, pw in ENGINE_CASES:
            want = ref.propagate(l, r, d, ph, pw)
            if (d >= 0).all():
                assert_same(e.propagate(l, r, d, ph, pw, 15), want, f"engine {engine} Propagate {name}")
            else:
                with pytest.raises(pm.PmError) as err:
                    e.propagate(l, r, d, ph, pw, 15)
                assert err.value.status == pm.PM_ERR_INVALID_ARG and ">= 0" in str(err.value), name
                refused += 1
            assert_same(e.remove_background(l, r, d, ph, pw, 1.5), ref.remove_background(l, r, d, ph, pw, 1.5),
                        f"engine {engine} RemoveBackground {name} / 1.5")
            assert_same(e.remove_background(l, r, want, ph, pw, 2.0), ref.remove_background(l, r, want, ph, pw, None),
                        f"engine {engine} RemoveBackground {name} / default")
        assert refused >= len(WINDOWS)
        # the refusal leaves the handle usable, and NaN counts as not >= 0
        name, l, r, d, ph, pw = next(c for c in ENGINE_CASES if c[0] == "5x5-99x61-truth_noise")
        bad = d.copy()
        bad[30, 50] = np.nan
        with pytest.raises(pm.PmError):
            e.propagate(l, r, bad, ph, pw, 15)
        assert_same(e.propagate(l, r, d, ph, pw, 15), ref.propagate(l, r, d, ph, pw), "after a refusal")


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ENGINES)
def test_engine_recipe_equals_the_compiled_reference(ref, pm, oracle, synth, engine):
    for what, (l, r, seed) in (("fsl1 / fsr1", farmsim_inputs(oracle)), ("150x96", synthetic_recipe_inputs(synth))):
        rows, cols = l.shape
        p = pm.default_params(0, patchmatch_iters=4, bg_patch_w=3, bg_patch_h=3, win_by_factor=1.5, left_right_check=0,
                              engine=engine, **RECIPE_SCHEDULE)
        with pm.Engine(p, max_rows=rows, max_cols=cols) as e:
            dl, _ = e.match(l, r, seed, None)
        assert_same(dl, ref.recipe(l, r, seed), f"engine {engine}, the test's recipe on {what}")


# ---- (d) the stated tolerance: the reference with its own flags against its uncontracted build -------------------------
def read_profile():
    rec = {}
    for line in open(PROFILE):
        if line.startswith("#") or not line.strip():
            continue
        name, rest = line.split(":", 1)
        rec[name.strip()] = {k: int(v) for k, v in (kv.split("=") for kv in rest.split())}
    return rec


def test_contracted_functor_differs_on_a_known_input(ref, ref_contracted):
    """One 3x3 patch pair with ec = eg = 1/9 (one pixel of colour and one of gradient differ by 1).  Unfused, the blend
    0.7f * ec + (1 - 0.7f) * eg rounds each product and then the sum: 0x1.c71c74p-4.  With either product fused into the
    sum (one rounding less) it is 0x1.c71c72p-4, one ulp lower."""
    assert ref_contracted.contracted and not ref.contracted
    pl, gl = np.zeros((3, 3), np.uint8), np.zeros((3, 3), np.float32)
    pr, gr = pl.copy(), gl.copy()
    pr[0, 0], gr[0, 0] = 1, 1.0
    alpha, e = np.float32(0.7), np.float32(1.0 / 9.0)
    unfused = np.float32(alpha * e) + np.float32((np.float32(1) - alpha) * e)
    assert float(unfused) == float.fromhex("0x1.c71c74p-4")
    assert ref.functor(pl, pr, gl, gr) == float.fromhex("0x1.c71c74p-4")
    assert ref_contracted.functor(pl, pr, gl, gr) == float.fromhex("0x1.c71c72p-4")


@pytest.mark.parametrize("name", ["farmsim", "band"])
def test_contracted_reference_stays_within_the_recorded_tolerance(ref, ref_contracted, oracle, synth, name):
    """profiles/ref_contract_tolerance.txt (tools/ref_contract_tolerance.py) records, for the compiler named there, how
    many pixels of the left map move when the reference is built as its own CMakeLists builds it.  The counts are
    deterministic for one compiler; twice the record is room for another g++ contracting differently, not for noise."""
    rec = read_profile()[name]
    got = contraction_counts(ref, ref_contracted, tolerance_inputs(oracle, synth)[name])
    print(name, "recorded", rec, "measured", got)
    assert got["of"] == rec["of"]
    assert got["differ"] > 0, "nothing was contracted: the comparison is vacuous"
    for key in ("differ", "gt1px", "fgbg"):
        assert got[key] <= 2 * rec[key], (key, got, rec)


# ---- (e) fixtures recorded from the compiled reference (tests/golden/make_golden.py --reference) ------------------------
def _golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def _golden_windows(c):
    return [tuple(int(v) for v in w) for w in c["windows"]]


def test_oracle_reproduces_reference_held_golden(oracle):
    c = _golden("ref_propagate_61x99")
    assert "stand-in" in str(c["note"])
    ims = oracle.ImageSet(c["left"], c["right"])
    assert_same(ims.gl, c["gl"], "gradient, left")
    assert_same(ims.gr, c["gr"], "gradient, right")
    for i, (ph, pw) in enumerate(_golden_windows(c)):
        for literal in (False, True):
            assert_same(oracle.cpu_propagate(ims, c["seed"], ph, pw, literal=literal), c["out"][i], f"Propagate {ph}x{pw}")
        assert_same(oracle.cpu_remove_background(ims, c["out"][i], ph, pw, 1.5), c["out_bg"][i], f"RemoveBackground {ph}x{pw}")
    z = np.load(os.path.join(GOLDEN, "farmsim_fs1_376x240.npz"))
    c = _golden("ref_recipe_farmsim")
    for literal in (1, 0):
        assert_same(oracle_recipe(oracle, z["left"], z["right"], c["seed"], literal), c["disp"], "recipe on fsl1 / fsr1")


@pytest.mark.gpu
def test_engine_reproduces_reference_held_golden(pm):
    c = _golden("ref_propagate_61x99")
    rows, cols = c["left"].shape
    for engine in ENGINES:
        with _engine(pm, engine, rows, cols) as e:
            assert_same(e.gradient_magnitude(c["left"]), c["gl"], "gradient, left")
            for i, (ph, pw) in enumerate(_golden_windows(c)):
                assert_same(e.propagate(c["left"], c["right"], c["seed"], ph, pw, 15), c["out"][i],
                            f"engine {engine} Propagate {ph}x{pw}")
                assert_same(e.remove_background(c["left"], c["right"], c["out"][i], ph, pw, 1.5), c["out_bg"][i],
                            f"engine {engine} RemoveBackground {ph}x{pw}")
    z = np.load(os.path.join(GOLDEN, "farmsim_fs1_376x240.npz"))
    c = _golden("ref_recipe_farmsim")
    p = pm.default_params(0, patchmatch_iters=4, bg_patch_w=3, bg_patch_h=3, win_by_factor=1.5, left_right_check=0,
                          **RECIPE_SCHEDULE)
    with pm.Engine(p, max_rows=240, max_cols=376) as e:
        dl, _ = e.match(z["left"], z["right"], c["seed"], None)
    assert_same(dl, c["disp"], "recipe on fsl1 / fsr1")


def test_library_still_reproduces_reference_held_golden(ref):
    """Guards the stand-in (and the recipe's flags) against drift: the fixtures are what the library wrote once."""
    c = _golden("ref_propagate_61x99")
    assert_same(ref.compute_gradient(c["left"]), c["gl"], "gradient, left")
    assert_same(ref.compute_gradient(c["right"]), c["gr"], "gradient, right")
    for i, (ph, pw) in enumerate(_golden_windows(c)):
        assert_same(ref.propagate(c["left"], c["right"], c["seed"], ph, pw), c["out"][i], f"Propagate {ph}x{pw}")
        assert_same(ref.remove_background(c["left"], c["right"], c["out"][i], ph, pw, 1.5), c["out_bg"][i],
                    f"RemoveBackground {ph}x{pw}")
    z = np.load(os.path.join(GOLDEN, "farmsim_fs1_376x240.npz"))
    c = _golden("ref_recipe_farmsim")
    assert_same(ref.recipe(z["left"], z["right"], c["seed"]), c["disp"], "recipe on fsl1 / fsr1")
