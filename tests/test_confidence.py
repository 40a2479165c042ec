"""Matching confidence of a disparity map (include/pm/imaging.h: pm_disparity_confidence).

CPU tests pin the definition (tests/confidence_ref.py) against analytic cases and run the kernel's own per-thread code
(csrc/pm_confidence_body.hpp) on the host under ASan / UBSan, blocks forwards and backwards, through the LDS tile and through
the global-memory path.  GPU tests hold the kernels to the definition with tolerance 0, bit patterns compared -- every
operation of the definition is one IEEE rounding, the build uses -ffp-contract=off, and only integer addition crosses
workgroups -- with guard bands around every output.  Every disturbed-map case is first shown to be non-trivial ON THE
DEFINITION ALONE: enough measured pixels, a keep rule that keeps some and removes some, every verdict populated."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import confidence_ref as CF
import oracle_lib as O
from conftest import ROOT
from cpp_build import build_host_kernel
from host_run import assert_program_compares, dump_case

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_confidence as FC  # noqa: E402  (check_confidence: the device-against-definition comparison; the cases)

gpu = pytest.mark.gpu

INF = float("inf")
SHAPES = {"1x1": (1, 1), "1x7": (1, 7), "11x11": (11, 11), "37x53": (37, 53), "40x64": (40, 64), "48x96": (48, 96),
          "17x131": (17, 131), "9x300": (9, 300)}
WINDOWS = {"3x3": (3, 3), "5x5": (5, 5), "7x3": (7, 3), "11x11": (11, 11), "15x15": (15, 15)}
# the shape / window pairs at which the disturbed map must show every verdict (the others are too small for the shares)
CONDITIONS = (("48x96", "11x11"), ("37x53", "5x5"), ("40x64", "7x3"), ("17x131", "3x3"))
FAILS = (CF.FAIL_COST, CF.FAIL_MARGIN, CF.FAIL_BG, CF.FAIL_LR)


def shifted_pair(rows, cols, k, seed=5):
    """A textured right image and the left image that is the right one shifted by k columns: left(x) = right(x - k)."""
    rng = np.random.default_rng(seed)
    right = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    left = np.roll(right, k, axis=1)
    left[:, :k] = rng.integers(0, 256, (rows, k)).astype(np.uint8)
    return left, right


# ---- 1. the definition ------------------------------------------------------------------------------------------------
def test_definition_an_exact_shift_costs_nothing_and_beats_its_neighbours():
    k, pw, ph = 6, 5, 5
    left, right = shifted_pair(24, 48, k)
    d = np.full((24, 48), float(k), np.float32)
    w = CF.confidence(left, right, d, d, pw, ph)
    m = w["measured"]
    want = np.zeros_like(m)
    want[ph // 2:24 - ph // 2, pw // 2 + k:48 - pw // 2] = True  # interior and k <= x - pw / 2
    assert np.array_equal(m, want) and w["valid"].all()
    # away from the columns the shift filled with other texture and from the right border, one more column for the Sobel taps
    clean = m.copy()
    clean[:, :k + pw // 2 + 1] = False
    clean[:, 48 - pw // 2 - 1:] = False
    c0, margin, bg, lr = (w["measures"][i] for i in range(4))
    assert not FC.bits(c0[clean]).any() and (margin[clean] > 0).all() and (bg[clean] > 0).all()
    assert not FC.bits(lr[m]).any()  # against the constant right map
    assert (w["flags"][m] == CF.MEASURED).all() and not w["flags"][~m].any()
    assert tuple(w["counts"]) == (24 * 48, m.sum(), m.sum()) and np.array_equal(FC.bits(w["out"]), FC.bits(d))
    assert (c0[~m] == -1).all() and not FC.bits(margin[~m]).any() and not FC.bits(bg[~m]).any() and np.isposinf(lr[~m]).all()


def test_definition_a_map_two_off_fails_margin_or_cost():
    k, pw = 6, 5
    left, right = shifted_pair(24, 48, k)
    d = np.full((24, 48), float(k + 2), np.float32)
    w = CF.confidence(left, right, d, None, pw, pw, max_cost=10.0, min_margin=2.0)
    m = w["measured"]
    assert m.sum() > 500
    assert ((w["flags"][m] & (CF.FAIL_COST | CF.FAIL_MARGIN)) != 0).all() and not (w["flags"] & CF.FAIL_LR).any()
    assert w["counts"][2] == 0 and not FC.bits(w["out"][m]).any() and np.array_equal(w["out"][~m], d[~m])
    assert np.isposinf(w["measures"][3]).all()  # no right map: lr is +inf everywhere


def test_definition_side_rules():
    left, right = shifted_pair(9, 40, 3)
    ims, pw, y, x = O.ImageSet(left, right), 5, 4, 20
    hi = np.float32(x - pw // 2)
    cost = lambda d: np.float32(O.cpu_cost(ims, pw, pw, x, y, np.float32(d), literal=False))
    def at(value):
        d = np.zeros((9, 40), np.float32)
        d[y, x] = value
        w = CF.confidence(left, right, d, None, pw, pw)
        assert w["measured"].sum() == 1 and w["measures"][0][y, x] == cost(value)
        assert w["measures"][2][y, x] == np.float32(cost(0.0) - cost(value))
        return int(w["sides"][y, x]), w["measures"][1][y, x]
    f = np.float32
    assert at(0.5) == (1, f(cost(1.5) - cost(0.5)))                      # d < 1: no side M
    n, margin = at(1.0)                                                  # d == 1: dm == 0 exists
    assert n == 2 and margin == f(min(cost(2.0), cost(0.0)) - cost(1.0))
    assert at(hi) == (1, f(cost(hi - 1) - cost(hi)))                     # d == hi: no side P
    assert at(hi - f(0.5)) == (1, f(cost(hi - f(1.5)) - cost(hi - f(0.5))))  # hi - 1 < d < hi: no side P
    n, margin = at(hi - 1)                                               # d == hi - 1: dp == hi exists
    assert n == 2 and margin == f(min(cost(hi), cost(hi - 2)) - cost(hi - 1))
    # no side at all: d < 1 at the first interior column, where hi = 0 ... is not valid; hi - 1 < d < 1 needs hi < 1
    d = np.zeros((9, 40), np.float32)
    d[y, pw // 2 + 1] = 0.5  # hi = 1: dm < 0 and dp = 1.5 > hi
    w = CF.confidence(left, right, d, None, pw, pw)
    assert w["sides"][y, pw // 2 + 1] == 0 and FC.bits(w["measures"][1])[y, pw // 2 + 1] == 0 and w["measured"].sum() == 1


def test_definition_a_window_larger_than_the_image_measures_nobody():
    left, right = shifted_pair(11, 11, 2)
    d = np.full((11, 11), 1.0, np.float32)
    for pw, ph in ((13, 3), (3, 13), (15, 15)):
        w = CF.confidence(left, right, d, d, pw, ph, drop_unmeasured=0)
        assert tuple(w["counts"]) == (121, 0, 0) and not w["flags"].any() and np.array_equal(w["out"], d)
        assert not CF.confidence(left, right, d, d, pw, ph, drop_unmeasured=1)["out"].any()
    w = CF.confidence(left, right, d, d, 11, 11)  # the window fits once, at x = 5, where hi = 0 < d
    assert tuple(w["counts"]) == (121, 0, 0)


def test_definition_special_values_in_both_maps():
    left, right = shifted_pair(9, 40, 3)
    pw, y = 5, 4
    d = np.full((9, 40), 3.0, np.float32)
    specials = np.array([0.0, -0.0, -2.0, np.nan, np.inf], np.float32)
    d[y, 10:15] = specials
    d[y, 20] = np.float32(20 - pw // 2) + np.float32(0.5)  # hi + a half
    for drop in (0, 1):
        w = CF.confidence(left, right, d, None, pw, pw, drop_unmeasured=drop)
        assert w["valid"][y, 10:15].tolist() == [False] * 4 + [True] and not w["measured"][y, 10:15].any()
        assert w["valid"][y, 20] and not w["measured"][y, 20] and not w["flags"][y, 20]
        assert np.array_equal(FC.bits(w["out"])[y, 10:14], FC.bits(specials)[:4])  # invalid pixels keep their bits
        keeps = FC.bits(d)[y, [14, 20]] if not drop else np.zeros(2, np.uint32)
        assert np.array_equal(FC.bits(w["out"])[y, [14, 20]], keeps)
        assert w["counts"][0] == d.size - 4 and w["counts"][1] == w["measured"].sum() == w["counts"][2]
    # D_r: 0, NaN and a negative give lr = +inf, +inf gives |inf - d| = +inf: all fail any finite max_lr_diff, pass +inf
    r = np.full((9, 40), 3.0, np.float32)
    r[y, 17:21] = (0.0, np.nan, np.inf, -1.0)  # q = x - 3: the pixels x = 20 .. 23 look there
    d = np.full((9, 40), 3.0, np.float32)
    w = CF.confidence(left, right, d, r, pw, pw, max_lr_diff=1e30)
    assert np.isposinf(w["measures"][3][y, 20:24]).all() and (w["flags"][y, 20:24] == CF.MEASURED | CF.FAIL_LR).all()
    assert (w["flags"][y, 24:30] == CF.MEASURED).all() and not FC.bits(w["measures"][3][y, 24:30]).any()
    w = CF.confidence(left, right, d, r, pw, pw, max_lr_diff=INF)
    assert (w["flags"][w["measured"]] == CF.MEASURED).all()


def test_definition_each_threshold_at_its_ends():
    left, right, dl, dr = FC.disturbed_case(37, 53, 5, 5)
    n = CF.confidence(left, right, dl, dr, 5, 5)["counts"][1]
    passing = dict(max_cost=INF, min_margin=-INF, min_bg_margin=-INF, max_lr_diff=INF)
    assert CF.confidence(left, right, dl, dr, 5, 5, **passing)["counts"][2] == n
    for (name, end), bit in zip((("max_cost", -INF), ("min_margin", INF), ("min_bg_margin", INF), ("max_lr_diff", -INF)), FAILS):
        w = CF.confidence(left, right, dl, dr, 5, 5, **dict(passing, **{name: end}))
        assert w["counts"][2] == 0 and (w["flags"][w["measured"]] == CF.MEASURED | bit).all(), name
    w = CF.confidence(left, right, dl, None, 5, 5, **dict(passing, max_lr_diff=-INF))  # read only with the right map
    assert w["counts"][2] == n


@functools.lru_cache(maxsize=None)
def _case(shape, window):
    rows, cols = SHAPES[shape]
    return FC.disturbed_case(rows, cols, *WINDOWS[window])


@functools.lru_cache(maxsize=None)
def _want(shape, window, with_right=True, drop=0):
    left, right, dl, dr = _case(shape, window)
    return CF.confidence(left, right, dl, dr if with_right else None, *WINDOWS[window], drop_unmeasured=drop, **FC.THRESHOLDS)


@pytest.mark.parametrize("shape,window", CONDITIONS)
def test_conditions_every_verdict_occurs_on_the_disturbed_map(shape, window):
    w = _want(shape, window)
    m = w["measured"]
    n = int(m.sum())
    share = lambda bit: float(((w["flags"][m] & bit) != 0).mean())
    print(shape, window, "measured %.3f kept %.3f" % (n / m.size, w["kept"].sum() / n), "FAIL shares",
          [round(share(b), 3) for b in FAILS], "sides", np.bincount(w["sides"][m], minlength=3))
    assert n >= 0.4 * m.size
    assert 0.2 <= w["kept"].sum() / n <= 0.8
    for bit in FAILS:
        assert 0.05 <= share(bit) <= 0.95, bit
    assert (np.bincount(w["sides"][m], minlength=3) > 0).all()


def test_conditions_nothing_is_measured_at_11x11_under_an_11x11_window():
    assert tuple(_want("11x11", "11x11")["counts"][1:]) == (0, 0)


# ---- 2. the kernel's own per-thread code, run on the host ------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_confidence_exe(tmp_path_factory):
    """tests/cpp/confidence_host_main.cpp: csrc/pm_confidence_body.hpp compiled for the host alone, with the sanitizers."""
    return build_host_kernel(tmp_path_factory.mktemp("confidencehost") / "confidence_host_main", "confidence_host_main.cpp")


def _dump_case(path, left, right, dl, dr, pw, ph, with_right, drop, functor=(0.7, 50.0, 20.0), **thresholds):
    want = CF.confidence(left, right, dl, dr if with_right else None, pw, ph, drop_unmeasured=drop, functor=functor, **thresholds)
    t = dict(dict(max_cost=INF, min_margin=-INF, min_bg_margin=-INF, max_lr_diff=INF), **thresholds)
    dump_case(path, [*dl.shape, pw, ph, t["max_cost"], t["min_margin"], t["min_bg_margin"], t["max_lr_diff"], drop, int(with_right),
                     *(np.float32(v) for v in functor)],
              left=left, right=right, disp_l=dl, disp_r=dr, want_out=want["out"], want_measures=want["measures"],
              want_flags=want["flags"], want_counts=want["counts"])
    return want


def test_kernel_code_on_the_host_equals_the_definition(host_confidence_exe, tmp_path):
    """Every thread of both launches over whole maps on the CPU -- forwards, backwards, in place, every block down the
    global-memory path, the counts alone: all outputs equal the .npy dumps of the definition byte for byte, and
    AddressSanitizer / UBSan see every access into buffers (a block's LDS tile too) of exactly the size the stage may touch.
    Five shapes x the windows 3, 7x3 and 11, the disturbed map with special values, and the ramp that overflows the tile."""
    kept, k, last = 0, 0, None
    for shape in ("1x1", "1x7", "37x53", "17x131", "9x300"):
        for window in ("3x3", "7x3", "11x11"):
            left, right, dl, dr = _case(shape, window)
            dl, dr = dl.copy(), dr.copy()
            m = min(FC.SPECIALS.size, dl.size - 1)
            dl.ravel()[:m] = FC.SPECIALS[:m]
            dr.ravel()[dl.size - m:] = FC.SPECIALS[:m]
            last = str(tmp_path / ("case%d" % k))
            kept += int(_dump_case(last, left, right, dl, dr, *WINDOWS[window], k % 3 != 2, k % 2, **FC.THRESHOLDS)["counts"][2])
            r = subprocess.run([host_confidence_exe, last], capture_output=True, text=True)
            assert r.returncode == 0, (shape, window, r.stderr[-3000:])
            k += 1
    assert kept > 1500
    d = str(tmp_path / "ramp")
    left, right, dl, dr = FC.ramp_case(9, 300, 3)
    want = _dump_case(d, left, right, dl, dr, 3, 3, True, 0, functor=(0.5, 30.0, 40.0), **FC.THRESHOLDS)
    r = subprocess.run([host_confidence_exe, d], capture_output=True, text=True)
    tiles = -(-9 // 8) * -(-300 // 32)
    assert r.returncode == 0 and want["counts"][1] > 2000, r.stderr[-3000:]
    assert int(re.search(r"tiled blocks: (\d+)", r.stdout).group(1)) < tiles  # some blocks took the global-memory path unasked
    # the program does compare: one flipped bit in an expectation is a mismatch, not a pass
    assert_program_compares(host_confidence_exe, last,
                            [("want_measures", np.uint32, "measures differs"), ("want_flags", np.uint8, "flags differs"),
                             ("want_out", np.uint32, "out differs"), ("want_counts", np.int32, "counts differs")])


def test_headers_declare_and_the_library_exports_the_confidence_functions(pm):
    text = open(os.path.join(ROOT, "include", "pm", "imaging.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    testing = open(os.path.join(ROOT, "include", "pm", "testing.h")).read()
    lib = pm.load()
    assert re.search(r"\bint\s+pm_disparity_confidence\s*\(\s*pm_handle\s*\*", text)
    assert "typedef struct pm_confidence_options" in text
    assert re.search(r"\bvoid\s+pm_debug_confidence_constants\s*\(\s*int\s*\*", testing)
    for name in ("pm_disparity_confidence", "pm_debug_confidence_constants"):
        assert name in pm.EXPORTS and hasattr(lib, name)
    assert C.sizeof(pm.PmConfidenceOptions) == 28
    assert (pm.PM_CONF_MEASURED, pm.PM_CONF_FAIL_COST, pm.PM_CONF_FAIL_MARGIN, pm.PM_CONF_FAIL_BG, pm.PM_CONF_FAIL_LR) == (
        CF.MEASURED, CF.FAIL_COST, CF.FAIL_MARGIN, CF.FAIL_BG, CF.FAIL_LR) == (1, 2, 4, 8, 16)
    for name, value in zip(("MEASURED", "FAIL_COST", "FAIL_MARGIN", "FAIL_BG", "FAIL_LR"), (1, 2, 4, 8, 16)):
        assert re.search(r"PM_CONF_%s\s*=\s*%d\b" % (name, value), text)
    assert pm.confidence_constants() == (32, 8, 224)
    assert re.search(r"#define\s+PM_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "pm", "patchmatch.h")).read())
    stages = open(os.path.join(ROOT, "ocean-perception_amd", "csrc", "pm_stages.hip")).read()
    assert '#include "pm_confidence.hpp"' in stages  # the kernels live in that unit alone
    for f in os.listdir(os.path.join(ROOT, "ocean-perception_amd", "csrc")):
        if f.endswith(".hip") and f != "pm_stages.hip":
            assert "pm_confidence" not in open(os.path.join(ROOT, "ocean-perception_amd", "csrc", f)).read(), f


# ---- 3. device parity ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        yield e


@gpu
@pytest.mark.parametrize("window", list(WINDOWS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_confidence_equals_the_definition(pm, engine, shape, window):
    """Eight shapes (one pixel, one row, a shape the 11x11 window fits once, rows and columns that are no multiple of the tile,
    several tiles both ways, a row of ten tiles with a ragged tail) x five windows (four templated or general squares, one
    that is not square): the map, the four measures, the flags, d_counts and the host counts at tolerance 0, with the right
    map; then without it and with drop_unmeasured."""
    import torch
    left, right, dl, dr = _case(shape, window)
    FC.check_confidence(torch, engine, left, right, dl, dr, *WINDOWS[window], want=_want(shape, window), **FC.THRESHOLDS)
    FC.check_confidence(torch, engine, left, right, dl, None, *WINDOWS[window], want=_want(shape, window, False, 1),
                        drop_unmeasured=1, **FC.THRESHOLDS)


@gpu
def test_each_output_alone_in_place_and_an_unaligned_image(pm, engine):
    import torch
    left, right, dl, dr = _case("37x53", "5x5")
    want = _want("37x53", "5x5")
    for only in FC.OUTPUTS:
        FC.check_confidence(torch, engine, left, right, dl, dr, 5, 5, outputs=(only,), want=want, **FC.THRESHOLDS)
    FC.check_confidence(torch, engine, left, right, dl, dr, 5, 5, in_place=True, want=want, **FC.THRESHOLDS)
    FC.check_confidence(torch, engine, left, right, dl, dr, 5, 5, outputs=("out",), in_place=True, want=want, **FC.THRESHOLDS)
    for offset in (1, 2, 3):
        FC.check_confidence(torch, engine, left, right, dl, dr, 5, 5, image_offset=offset, want=want, **FC.THRESHOLDS)


@gpu
@pytest.mark.parametrize("window", ["3x3", "11x11", "15x15"])
def test_a_ramp_that_overflows_the_target_tile_takes_the_global_path(pm, engine, window):
    """d = 1 beside d = x - pw / 2 - 1: from about column 224 on a tile's target span exceeds what the LDS holds.  By the
    exported launch constants some tiles of the case do fall back and some do not; both give the definition."""
    import torch
    pw = WINDOWS[window][0]
    left, right, dl, dr = FC.ramp_case(24, 300, pw)
    want = CF.confidence(left, right, dl, dr, pw, pw, **FC.THRESHOLDS)
    constants = pm.confidence_constants()
    tiles = -(-24 // constants[1]) * -(-300 // constants[0])
    n = FC.fallback_tiles(dl, want["measured"], pw, constants)
    interior = (24 - pw + 1) * (300 - pw + 1)  # both values of the ramp lie in the measured domain from the second interior column on
    assert 2 <= n <= tiles - 2 and want["counts"][1] > 0.9 * interior, (n, tiles, want["counts"])
    FC.check_confidence(torch, engine, left, right, dl, dr, pw, pw, want=want, **FC.THRESHOLDS)


@gpu
def test_special_values_in_both_maps(pm, engine):
    import torch
    rng = np.random.default_rng(9)
    left, right, dl, dr = _case("37x53", "5x5")
    dl, dr = dl.copy(), dr.copy()
    x = np.arange(53, dtype=np.float32)[None, :].repeat(37, 0)
    for a in (dl, dr):
        pick = rng.random(a.shape) < 0.15
        a[pick] = rng.choice(FC.SPECIALS, int(pick.sum()))
    pick = rng.random(dl.shape) < 0.05
    dl[pick] = (x - np.float32(2) + np.float32(0.5))[pick]  # hi + a half
    dl.ravel()[:FC.SPECIALS.size] = FC.SPECIALS
    for drop in (0, 1):
        want = FC.check_confidence(torch, engine, left, right, dl, dr, 5, 5, drop_unmeasured=drop, **FC.THRESHOLDS)
        assert 0 < want["counts"][2] < want["counts"][1] < want["counts"][0] and np.isnan(want["out"]).any()
    for name, end in (("max_cost", -INF), ("min_margin", INF), ("min_bg_margin", INF), ("max_lr_diff", -INF), ("max_lr_diff", INF)):
        FC.check_confidence(torch, engine, left, right, dl, dr, 5, 5, **{name: end})


@gpu
def test_invalid_arguments_are_named_and_nothing_is_enqueued(pm, engine):
    """PM_ERR_INVALID_ARG with pm_last_error naming the argument; every output keeps its guard pattern."""
    import torch
    rows, cols = 16, 24
    lib, h = engine.lib, engine.h
    img = torch.full((2, rows, cols), 7, dtype=torch.uint8, device="cuda")
    disp = torch.full((2, rows, cols), 2.0, dtype=torch.float32, device="cuda")
    outs = {k: FC.Guarded(torch, n) for k, n in (("out", 4 * rows * cols), ("meas", 16 * rows * cols), ("flags", rows * cols), ("c", 12))}
    host = (C.c_int * 3)(-5, -5, -5)
    UNSET = object()

    def call(opt=(5, 5, 10.0, 2.0, 5.0, 1.0, 0), left=UNSET, right=UNSET, dl=UNSET, dr=UNSET, shape=(rows, cols), out=UNSET,
             meas=UNSET, flags=UNSET, c=UNSET, hc=host):
        o = pm.PmConfidenceOptions(*opt) if opt is not None else None
        pick = lambda v, default: default if v is UNSET else v
        return lib.pm_disparity_confidence(h, C.byref(o) if o is not None else None, pick(left, img[0].data_ptr()),
                                           pick(right, img[1].data_ptr()), pick(dl, disp[0].data_ptr()), pick(dr, disp[1].data_ptr()),
                                           shape[0], shape[1], pick(out, outs["out"].ptr), pick(meas, outs["meas"].ptr),
                                           pick(flags, outs["flags"].ptr), pick(c, outs["c"].ptr), hc)

    def refused(rc, word, status=pm.PM_ERR_INVALID_ARG):
        text = lib.pm_last_error(h).decode()
        assert rc == status and word in text and "pm_disparity_confidence" in text, (rc, word, text)

    assert lib.pm_disparity_confidence(None, None, None, None, None, None, rows, cols, None, None, None, None, None) == pm.PM_ERR_INVALID_ARG
    refused(call(opt=None), "options")
    refused(call(left=None), "d_left")
    refused(call(right=None), "d_right")
    refused(call(dl=None), "d_disp_l")
    refused(call(out=None, meas=None, flags=None, c=None, hc=None), "no output")
    for bad in (1, 2, 4, 17, -3, 0):
        refused(call(opt=(bad, 5, 10.0, 2.0, 5.0, 1.0, 0)), "patch_w")
        refused(call(opt=(5, bad, 10.0, 2.0, 5.0, 1.0, 0)), "patch_h")
    for i, name in enumerate(("max_cost", "min_margin", "min_bg_margin", "max_lr_diff")):
        opt = [5, 5, 10.0, 2.0, 5.0, 1.0, 0]
        opt[2 + i] = np.nan
        refused(call(opt=tuple(opt)), name)
    for bad in (-1, 2):
        refused(call(opt=(5, 5, 10.0, 2.0, 5.0, 1.0, bad)), "drop_unmeasured")
    refused(call(shape=(0, cols)), "empty")
    refused(call(shape=(rows, 0)), "empty")
    refused(call(shape=(rows, -3)), "empty")
    refused(call(out=disp[1].data_ptr()), "d_disp_r")
    refused(call(shape=(70000, 40000)), "exceed", pm.PM_ERR_SIZE)
    engine.synchronize()
    for buf in outs.values():
        buf.read(np.uint8, 0)
    assert tuple(host) == (-5, -5, -5) and (disp.cpu().numpy() == 2.0).all() and (img.cpu().numpy() == 7).all()
    # and the same arguments made good do run: a flat pair measures every interior pixel with d <= hi
    measured = (rows - 4) * (cols - 4 - 2)
    assert call() == pm.PM_OK and tuple(host)[:2] == (rows * cols, measured)
    assert call(dr=None) == pm.PM_OK and call(out=disp[0].data_ptr()) == pm.PM_OK  # no right map; in place


@gpu
def test_confidence_scratch_is_owned_by_the_handle(pm):
    """The counts and the two gradient planes are ONE handle-owned allocation through csrc/pm_devbuf.hpp: made on first use,
    grown for a larger image, reused for the same or a smaller one, gone with the handle."""
    import torch
    lib = pm.load()
    live = lambda: (lib.pm_debug_live_device_allocations(), lib.pm_debug_live_device_bytes())
    before = live()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        base = live()
        def run(rows, cols):
            img = torch.full((2, rows, cols), 9, dtype=torch.uint8, device="cuda")
            d = torch.full((rows, cols), 1.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            return e.disparity_confidence(img[0].data_ptr(), img[1].data_ptr(), d.data_ptr(), None, rows, cols, 5, want_counts=True)
        assert run(37, 53)[0] == 37 * 53
        first = live()
        assert first[0] == base[0] + 1 and first[1] - base[1] >= 16 + 5 * 37 * 53
        assert run(37, 53)[0] == 37 * 53 and live() == first  # a second call of the same size allocates nothing
        assert run(20, 31)[0] == 20 * 31 and live() == first
        assert run(100, 150)[0] == 100 * 150
        grown = live()
        assert grown[0] == first[0] and grown[1] > first[1]
        assert run(37, 53)[0] == 37 * 53 and live() == grown
    assert live() == before


@gpu
@pytest.mark.parametrize("kind", ["planes", "gpu-semantics", "functor"])
def test_the_stage_does_not_depend_on_the_handles_mode_or_semantics(pm, kind):
    """On a PM_MODE_PLANES handle and on a PM_SEM_GPU handle the stage gives the bits of the PM_SEM_CPU definition; a handle
    with another functor gives that functor's."""
    import torch
    left, right, dl, dr = _case("37x53", "5x5")
    kw = {"planes": dict(mode=pm.PM_MODE_PLANES, max_disp=32), "gpu-semantics": {},
          "functor": dict(functor_alpha=0.5, functor_tau_color=30.0, functor_tau_grad=40.0)}[kind]
    prm = pm.default_params(pm.PM_SEM_GPU if kind == "gpu-semantics" else pm.PM_SEM_CPU, patch=3 if kind == "gpu-semantics" else 7, **kw)
    with pm.Engine(prm, max_rows=64, max_cols=96) as e:
        want = FC.check_confidence(torch, e, left, right, dl, dr, 5, 5, want=None if kind == "functor" else _want("37x53", "5x5"),
                                   **FC.THRESHOLDS)
    if kind == "functor":
        assert not np.array_equal(want["measures"][0], _want("37x53", "5x5")["measures"][0])


# ---- 4. behind Match(), on the device maps --------------------------------------------------------------------------------
@gpu
def test_match_then_confidence_on_the_device_maps(pm, synth):
    """pm_match_device -> pm_disparity_confidence on the handle's stream, nothing copied: the result equals the definition on
    the downloaded maps, and c0 of every measured pixel is the cost the engine's own noise + cost stage reports for that map
    (pm_debug_noise_cost with amount < 0): the stage and the matcher agree on what a cost is."""
    import torch
    rows, cols, patch = 64, 96, 7
    p = synth.make_pair(3, rows=rows, cols=cols, n_points=40, dilate_factor=2)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    L, R, SL, SR = up(p["left"]), up(p["right"]), up(p["seed_l"]), up(p["seed_r"])
    D = torch.zeros((2, rows, cols), dtype=torch.float32, device="cuda")
    out = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    meas = torch.zeros((4, rows, cols), dtype=torch.float32, device="cuda")
    flags = torch.zeros((rows, cols), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pm.Engine(pm.default_params(0, patch=patch, patchmatch_iters=3), max_rows=rows, max_cols=cols) as e:
        e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), D[0].data_ptr(), D[1].data_ptr())
        n = e.disparity_confidence(L.data_ptr(), R.data_ptr(), D[0].data_ptr(), D[1].data_ptr(), rows, cols, patch,
                                   d_out=out.data_ptr(), d_measures=meas.data_ptr(), d_flags=flags.data_ptr(), want_counts=True,
                                   **FC.THRESHOLDS)
        e.synchronize()
        maps = D.cpu().numpy()
        _, plane = e.debug_noise_cost(p["left"], p["right"], maps[0], patch, patch, -1.0, 0,
                                      cost=np.full((rows, cols), -7.0, np.float32))
    want = CF.confidence(p["left"], p["right"], maps[0], maps[1], patch, patch, **FC.THRESHOLDS)
    m = want["measured"]
    assert want["counts"][1] > 0.25 * rows * cols and 0 < want["counts"][2] < want["counts"][1]
    assert np.array_equal(m[3:-3, 3:-3], maps[0][3:-3, 3:-3] > 0)  # every interior value Match() returns is measured
    assert n == tuple(int(v) for v in want["counts"])
    assert np.array_equal(FC.bits(out.cpu().numpy()), FC.bits(want["out"]))
    assert np.array_equal(FC.bits(meas.cpu().numpy()), FC.bits(want["measures"]))
    assert np.array_equal(flags.cpu().numpy(), want["flags"])
    assert np.array_equal(FC.bits(meas[0].cpu().numpy()[m]), FC.bits(np.ascontiguousarray(plane[m])))


@gpu
def test_fuzz_confidence_one_short_seeded_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_confidence.py"), "--cases", "12", "--seed", "4"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
