"""Sequence fusion: the newest left map refined by, and filled from, earlier maps of its sequence (include/pm/imaging.h:
pm_fuse_disparity).

CPU tests pin the definition (tests/fuse_ref.py) against analytic cases, show ON THE DEFINITION ALONE that the cases the
kernels are held to do fuse and fill (the error against the truth falls, most holes are filled, few fills are wrong), and run the
kernels' own per-thread code (csrc/pm_fuse_body.hpp) on the host under ASan / UBSan, blocks forwards and backwards.  GPU tests
hold the kernels to the definition with tolerance 0 -- every operation of the definition is one IEEE rounding, the build uses
-ffp-contract=off, and only integer maximum and integer addition cross workgroups -- with guard bands around every output."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import consistency_ref as CR
import fuse_ref as FU
from conftest import ROOT
from cpp_build import build_host_kernel
from host_run import assert_program_compares, dump_case, flat_motions
from pointcloud_ref import camera_for
from test_reproject import CAM, FXB, motions, two_level

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_fuse as FF  # noqa: E402  (check_fuse: the device-against-definition comparison)

gpu = pytest.mark.gpu

I3 = np.eye(3).ravel()
ZERO = np.zeros(3)
IDENT = (I3, ZERO)
SHAPES = {"1x1": (1, 1), "1x7": (1, 7), "37x53": (37, 53), "64x96": (64, 96), "17x131": (17, 131), "9x300": (9, 300)}
REAL = ("identity", "baseline", "advance", "yaw", "roll")  # the motions that leave something to see
THREE = ("identity", "baseline", "yaw")
MAX_DIFF = 0.75  # above the +-0.3 of the current map plus the +-0.3 of a disturbed source, below the steps of 4
OPT = dict(max_diff=MAX_DIFF, radius=0, min_consistent=1, max_conflicts=8, fill_max_diff=0.75)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float32))).astype(np.float64)


# ---- 1. the definition ------------------------------------------------------------------------------------------------
def test_definition_restates_the_consistency_stage_exactly():
    """The tap that fuse_ref chooses is consistency_ref's (same class at every pixel, every radius), the depths are the ones
    its projection formed, and classes, valid and kept counts are pm_filter_consistency's."""
    cur, cam, sources, mots, _ = fuse_case(37, 53, REAL)
    for radius in (0, 1, 2):
        for s, (R, t) in zip(sources, mots):
            cls, abs_e, _ = CR.classify(cur, s, cam, R, t, MAX_DIFF, radius)
            got, ds, ty, tx = FU.chosen_tap(cur, s, cam, R, t, MAX_DIFF, radius)
            assert np.array_equal(cls, got)
            seen, iu, iv, dp = CR.project(cur, cam, R, t)
            hit = got != CR.UNSEEN
            assert np.array_equal(np.abs(ds.astype(np.float64) - dp.astype(np.float64))[hit], abs_e[hit])
            assert np.array_equal(s[ty, tx][hit], ds[hit]) and (np.abs(ty - iv)[hit] <= radius).all() and (np.abs(tx - iu)[hit] <= radius).all()
            Z, Zn = FU.depths(cur, cam, R, t)
            assert np.array_equal((np.float64(cam[0]) * np.float64(cam[4]) / Zn).astype(np.float32)[seen], dp[seen])
        want = FU.fuse(cur, sources, cam, mots, max_diff=MAX_DIFF, radius=radius, min_consistent=2, max_conflicts=0)
        ref = CR.filter_consistency(cur, sources, cam, mots, MAX_DIFF, radius, 2, 0)
        assert np.array_equal(want["per_source"], ref["per_source"]) and tuple(want["counts"][:2]) == tuple(ref["counts"])
        assert np.array_equal(want["out"] == 0, ref["out"] == 0) and 0 < ref["counts"][1] < ref["counts"][0]


def test_definition_a_source_equal_to_the_map_changes_nothing():
    """Analytic case 1: R = I, t = 0, the map as its own source: within 1 binary32 ulp of d, two observations."""
    rng = np.random.default_rng(11)
    for _ in range(10):
        d = rng.uniform(0.01, 128.0, (48, 80)).astype(np.float32)
        d[rng.random((48, 80)) < 0.2] = 0.0
        out = FU.fuse(d, [d], CAM, [IDENT], max_diff=0.0, radius=0)
        v = d > 0
        assert (np.abs(out["out"].astype(np.float64) - d)[v] <= ulp32(d)[v]).all() and (out["count"][v] == 2).all()
        assert (out["spread"][v] <= ulp32(d)[v]).all() and (out["flags"][v] == 7).all()
        assert np.array_equal(FF.bits(out["out"])[~v], FF.bits(d)[~v]) and not out["count"][~v].any() and not out["flags"][~v].any()
        assert tuple(out["counts"]) == (v.sum(), v.sum(), v.sum(), 0)


def test_definition_a_constant_offset_is_halved_and_weights_shift_it():
    """Analytic case 2: a source off by e under identity gives d + e / 2; with weights 1 and 3, d + 3 e / 4."""
    d = np.random.default_rng(3).uniform(8.0, 12.0, (48, 80)).astype(np.float32)
    src = (d + np.float32(0.5)).astype(np.float32)
    out = FU.fuse(d, [src], CAM, [IDENT], max_diff=1.0, radius=0)
    mean = (d.astype(np.float64) + src) / 2
    assert (np.abs(out["out"] - mean) <= ulp32(mean)).all() and (out["count"] == 2).all()
    assert (np.abs(out["spread"] - 0.5) <= 2 * ulp32(d)).all()
    w0, w1 = np.ones((48, 80), np.float32), np.full((48, 80), 3.0, np.float32)
    out = FU.fuse(d, [src], CAM, [IDENT], w0, [w1], max_diff=1.0, radius=0)
    mean = (d.astype(np.float64) + 3 * src.astype(np.float64)) / 4
    assert (np.abs(out["out"] - mean) <= ulp32(mean)).all()


def test_definition_an_advance_reproduces_the_map_in_its_own_ray():
    """Analytic case 3: a constant-20 plane, the source 10 % of the range nearer holds 20 / 0.9: o_k is 20 again."""
    d = np.full((48, 80), 20.0, np.float32)
    t = (0.0, 0.0, -0.1 * (FXB / 20.0))
    src = np.full((48, 80), np.float32(20.0 / 0.9), np.float32)
    out = FU.fuse(d, [src], CAM, [(I3, t)], max_diff=1e-5, radius=0, min_consistent=0)
    seen = CR.project(d, CAM, I3, t)[0]
    assert 0.5 < seen.mean() < 1.0  # the image spreads about the principal point: its rim leaves
    assert np.array_equal(out["count"], np.where(seen, 2, 1)) and np.array_equal(out["flags"], np.where(seen, 7, 3))
    assert (np.abs(out["out"].astype(np.float64) - 20.0) <= 2 * ulp32(20.0)).all() and out["spread"].max() <= 4e-6
    assert np.array_equal(FF.bits(out["out"])[~seen], FF.bits(d)[~seen])  # alone with weight 1: num / den is d exactly


def test_definition_every_special_weight():
    """Analytic case 4: 0, -0.0, -1, NaN, +inf, -inf count as 0 and that observation does not take part; a subnormal, 0.25
    and 3 count as they are."""
    W = FF.WEIGHT_SPECIALS
    n = W.size
    cam = camera_for(1, n)
    d, src, ones = np.full((1, n), 10.0, np.float32), np.full((1, n), 11.0, np.float32), np.ones((1, n), np.float32)
    good = np.array([False] * 6 + [True] * 3)
    assert np.array_equal(FU.weight64(W) > 0, good)
    own = FU.fuse(d, [src], cam, [IDENT], W[None], [ones], max_diff=2.0, radius=0)
    assert np.array_equal(own["count"][0], np.where(good, 2, 1)) and (own["flags"] == 7).all()
    want = np.where(good, (FU.weight64(W) * 10.0 + 11.0) / (FU.weight64(W) + 1.0), 11.0)
    assert (np.abs(own["out"][0] - want) <= ulp32(want)).all() and (own["spread"][0][~good] == 0).all()
    theirs = FU.fuse(d, [src], cam, [IDENT], ones, [W[None]], max_diff=2.0, radius=0)
    assert np.array_equal(theirs["count"][0], np.where(good, 2, 1)) and np.array_equal(theirs["flags"][0], np.where(good, 7, 3))
    want = np.where(good, (10.0 + FU.weight64(W) * 11.0) / (1.0 + FU.weight64(W)), 10.0)
    assert (np.abs(theirs["out"][0] - want) <= ulp32(want)).all()
    assert np.array_equal(FF.bits(theirs["out"])[0][~good], FF.bits(d)[0][~good])
    none = FU.fuse(d, [src], cam, [IDENT], W[None], [W[None]], max_diff=2.0, radius=0)
    assert np.array_equal(FF.bits(none["out"])[0][~good], FF.bits(d)[0][~good])  # den is not > 0: the input bits
    assert not none["count"][0][~good].any() and not FF.bits(none["spread"])[0][~good].any() and (none["flags"][0][~good] == 3).all()
    null = FU.fuse(d, [src], cam, [IDENT], None, [None], max_diff=2.0, radius=0)
    assert np.array_equal(FF.bits(null["out"]), FF.bits(FU.fuse(d, [src], cam, [IDENT], ones, [ones], max_diff=2.0, radius=0)["out"]))


def test_definition_the_fill_vote():
    """Analytic case 5: three sources under identity, one nearer by more than fill_max_diff: with fill_min_sources 1 the
    nearest alone fills, with 2 nothing does; three that agree are averaged in order."""
    cam = camera_for(5, 7)
    d = np.zeros((5, 7), np.float32)
    d[0, :4] = [-0.0, -3.0, np.nan, 0.0]
    src = [np.full((5, 7), v, np.float32) for v in (10.0, 10.2, 14.0)]
    fill = lambda m, s=src: FU.fuse(d, s, cam, [IDENT] * 3, max_diff=1.0, radius=0, fill_min_sources=m, fill_max_diff=0.75)
    assert np.array_equal(FF.bits(FU.fill_splats(src, cam, [IDENT] * 3)), FF.bits(np.stack(src)))  # identity: the maps themselves
    one = fill(1)
    assert (one["out"] == 14.0).all() and (one["count"] == 1).all() and not FF.bits(one["spread"]).any() and (one["flags"] == 8).all()
    assert tuple(one["counts"]) == (0, 0, 0, 35)
    two = fill(2)
    assert np.array_equal(FF.bits(two["out"]), FF.bits(d)) and not two["count"].any() and not two["flags"].any() and two["counts"][3] == 0
    off = fill(0)
    assert np.array_equal(FF.bits(off["out"]), FF.bits(d)) and off["splats"] is None
    agree = [src[0], src[1], np.full((5, 7), 10.5, np.float32)]
    for m in (1, 2, 3):
        three = fill(m, agree)
        acc = (np.float64(np.float32(10.0)) + np.float64(np.float32(10.2))) + np.float64(np.float32(10.5))
        assert (three["out"] == np.float32(acc / 3.0)).all() and (three["count"] == 3).all() and (three["spread"] == np.float32(0.5)).all()
    gap = [src[0], np.zeros((5, 7), np.float32), src[2]]  # a source without a value there is no candidate
    assert (fill(1, gap)["count"] == 1).all() and fill(2, gap)["counts"][3] == 0


def test_definition_a_removed_pixel_is_never_filled():
    """Analytic case 6: a valid pixel that is not KEPT becomes +0.0 although the sources do carry a value to it."""
    cam = camera_for(5, 7)
    d = np.full((5, 7), 10.0, np.float32)
    through = np.full((5, 7), 2.0, np.float32)  # seen through: CONFLICT
    out = FU.fuse(d, [through, through], cam, [IDENT] * 2, max_diff=1.0, radius=0, min_consistent=0, max_conflicts=1,
                  fill_min_sources=1, fill_max_diff=0.75)
    assert (out["splats"] == 2.0).all() and not FF.bits(out["out"]).any() and (out["flags"] == FU.VALID).all()
    assert tuple(out["counts"]) == (35, 0, 0, 0) and (out["count"] == 1).all()
    out = FU.fuse(d, [through, through], cam, [IDENT] * 2, max_diff=1.0, radius=0, min_consistent=0, max_conflicts=8)
    assert np.array_equal(FF.bits(out["out"]), FF.bits(d)) and (out["flags"] == 3).all()  # 0 and 8 remove nothing


def test_definition_flag_bits_and_the_four_counts():
    """Analytic case 7: one row with a fused, a kept-but-alone, a removed, a filled and an empty pixel."""
    cam = camera_for(1, 5)
    d = np.array([[10.0, 10.0, 10.0, 0.0, 0.0]], np.float32)
    s = np.array([[10.5, 0.0, 2.0, 9.0, 0.0]], np.float32)
    out = FU.fuse(d, [s], cam, [IDENT], max_diff=1.0, radius=0, min_consistent=0, max_conflicts=0, fill_min_sources=1)
    assert out["flags"][0].tolist() == [FU.VALID | FU.KEPT | FU.FUSED, FU.VALID | FU.KEPT, FU.VALID, FU.FILLED, 0]
    assert (FU.VALID, FU.KEPT, FU.FUSED, FU.FILLED) == (1, 2, 4, 8) and tuple(out["counts"]) == (3, 2, 1, 1)
    assert out["count"][0].tolist() == [2, 1, 1, 1, 0] and out["out"][0].tolist() == [10.25, 10.0, 0.0, 9.0, 0.0]
    assert out["count"].dtype == np.uint8 and out["flags"].dtype == np.uint8 and out["counts"].dtype == np.int32


def test_definition_an_infinite_pixel_gives_the_canonical_nan():
    d = np.full((3, 4), np.inf, np.float32)
    out = FU.fuse(d, [d], camera_for(3, 4), [IDENT], max_diff=1.0, radius=0, min_consistent=0, max_conflicts=8)
    assert (FF.bits(out["spread"]) == 0x7FC00000).all() and (FF.bits(out["out"]) == FF.bits(d)).all()


# ---- the cases the kernels are held to, and what makes them worth running ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def fuse_case(rows, cols, names, cam=None, very_near=False):
    """truth: two_level without holes; the current map: truth + U(-0.3, 0.3) with 8 % of its pixels lost; one source per named
    motion: the TRUTH carried into its view and disturbed (tools/fuzz_consistency.py: disturbed_source, seed 7 + k)."""
    cam = camera_for(rows, cols) if cam is None else cam
    truth = two_level(rows, cols, seed=rows + cols, zeros=0.0, very_near=very_near)
    rng = np.random.default_rng(5)
    cur = (truth + rng.uniform(-0.3, 0.3, truth.shape).astype(np.float32)).astype(np.float32)
    cur[rng.random(truth.shape) < 0.08] = 0.0
    table = motions(cam, FXB / 6.0)
    mots = tuple(table[name] for name in names)
    sources = tuple(FF.disturbed_source(truth, cam, m, seed=7 + k) for k, m in enumerate(mots))
    return cur, cam, sources, mots, truth


def _names(motion, n):
    """The first source under `motion`, the others under the real motions in turn."""
    first = REAL.index(motion) + 1 if motion in REAL else 0
    return (motion,) + tuple(REAL[(first + j) % len(REAL)] for j in range(n - 1))


@functools.lru_cache(maxsize=None)
def _want(shape, names, radius=0, fill=None, weighted=False):
    rows, cols = SHAPES[shape]
    cur, cam, sources, mots, _ = fuse_case(rows, cols, names, very_near="behind" in names)
    n = len(names)
    w, ws = _weights(rows, cols, n) if weighted else (None, None)
    return FU.fuse(cur, sources, cam, mots, w, ws, **dict(OPT, radius=radius), fill_min_sources=min(2, n) if fill is None else fill)


@functools.lru_cache(maxsize=None)
def _weights(rows, cols, n):
    rng = np.random.default_rng(rows * cols + n)
    return FF.random_weight(rng, rows, cols), tuple(FF.random_weight(rng, rows, cols) if k % 3 != 1 else None for k in range(n))


def _quality(shape, names):
    rows, cols = SHAPES[shape]
    cur, _, _, _, truth = fuse_case(rows, cols, names)
    want = _want(shape, names)
    f, holes = want["fused"], cur == 0
    ratio = np.abs(want["out"] - truth)[f].mean() / np.abs(cur - truth)[f].mean()
    bad = int((want["filled"] & (np.abs(want["out"] - truth) > 0.75)).sum())
    return ratio, int(want["filled"].sum()), int(holes.sum()), bad


def test_conditions_fusion_halves_the_error_and_fills_most_holes():
    """37x53 and 64x96, sources identity / baseline / yaw: mean |error| of the fused pixels after / before <= 0.65 (prototype:
    0.150 -> 0.077), at least 75 % of the holes filled (136 of 156, 409 of 461), at most 5 % of the fills further than 0.75
    from the truth (0 and 7)."""
    for shape in ("37x53", "64x96"):
        ratio, filled, holes, bad = _quality(shape, THREE)
        print(shape, "error ratio %.3f, filled %d of %d, bad fills %d" % (ratio, filled, holes, bad))
        assert ratio <= 0.65 and filled >= 0.75 * holes and bad <= 0.05 * filled, (shape, ratio, filled, holes, bad)


def test_conditions_thin_shapes_fuse_fill_and_leave_holes():
    for shape in ("17x131", "9x300"):
        want = _want(shape, THREE)
        rows, cols = SHAPES[shape]
        left = (fuse_case(rows, cols, THREE)[0] == 0) & ~want["filled"]
        print(shape, "fused", want["counts"][2], "filled", want["counts"][3], "not filled", left.sum())
        assert want["counts"][2] >= 1 and want["counts"][3] >= 1 and left.sum() >= 1
    want = _want("1x7", REAL)
    print("1x7", want["counts"])
    assert want["counts"][2] >= 1 and want["counts"][3] >= 1


# ---- 2. the kernels' own per-thread code, run on the host -------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_fuse_exe(tmp_path_factory):
    """tests/cpp/fuse_host_main.cpp: csrc/pm_fuse_body.hpp compiled for the host alone, with the sanitizers."""
    return build_host_kernel(tmp_path_factory.mktemp("fusehost") / "fuse_host_main", "fuse_host_main.cpp")


def _dump_case(path, cur, cam, sources, mots, weight, source_weights, radius, min_consistent, max_conflicts, fill_min, fill_max_diff):
    n = len(sources)
    want = FU.fuse(cur, sources, cam, mots, weight, source_weights, MAX_DIFF, radius, min_consistent, max_conflicts, fill_min, fill_max_diff)
    has = np.zeros(FU.MAX_SOURCES)
    has[:n] = [w is not None for w in source_weights]
    planes = [np.full(cur.shape, 7.0, np.float32) if w is None else w for w in [weight] + list(source_weights)]
    dump_case(path, [*cur.shape, *cam, n, radius, MAX_DIFF, min_consistent, max_conflicts, fill_min, fill_max_diff, weight is not None,
                     *has, *flat_motions(mots, FU.MAX_SOURCES)],
              disp=cur, sources=np.stack(sources).astype(np.float32), weights=np.stack(planes).astype(np.float32),
              **{"want_" + name: want[name] for name in ("out", "count", "spread", "flags", "counts")})
    return want


def test_kernel_code_on_the_host_equals_the_definition(host_fuse_exe, tmp_path):
    """Every thread of both launches over whole maps on the CPU, forwards, backwards, in place and with the counts alone: all
    five outputs equal the .npy dumps of the definition byte for byte, and AddressSanitizer / UBSan see every access into
    buffers of exactly the size the stage may touch (no splat scratch at all without a fill).  Six shapes x n = 1, 3, 8 x
    radius 0..2, the motions in turn, the fill on and off, weights given and null, special values in the current map, in the
    sources and in the weights."""
    names = REAL + ("behind", "gone")
    totals, k = np.zeros(4, np.int64), 0
    for shape in SHAPES:
        for n in (1, 3, 8):
            for radius in (0, 1, 2):
                rows, cols = SHAPES[shape]
                motion = names[k % len(names)]
                cur, cam, sources, mots, _ = fuse_case(rows, cols, _names(motion, n), very_near=motion == "behind")
                cur, sources = cur.copy(), [s.copy() for s in sources]
                m = min(FF.SPECIALS.size, cur.size - 1)
                cur.ravel()[:m] = FF.SPECIALS[:m]
                sources[-1].ravel()[cur.size - m:] = FF.SPECIALS[:m]
                w, ws = _weights(rows, cols, n) if k % 2 else (None, (None,) * n)
                fill = (0, min(2, n), 1)[k % 3]
                d = str(tmp_path / ("case%d" % k))
                totals += _dump_case(d, cur, cam, sources, mots, w, ws, radius, min(1, n), 8 if k % 4 else 0, fill, 0.75)["counts"]
                r = subprocess.run([host_fuse_exe, d], capture_output=True, text=True)
                assert r.returncode == 0, (shape, n, radius, motion, fill, r.stderr[-3000:])
                k += 1
    print("valid, kept, fused, filled:", totals)
    assert totals[2] > 10000 and totals[3] > 1000 and totals[1] < totals[0]
    # the program does compare: one flipped bit in an expectation is a mismatch, not a pass
    assert_program_compares(host_fuse_exe, str(tmp_path / "case31"),
                            [("want_" + name, dtype, name + " differs") for name, dtype in
                             (("spread", np.uint32), ("count", np.uint8), ("flags", np.uint8), ("out", np.uint32), ("counts", np.int32))])


def test_headers_declare_and_the_library_exports_the_fuse_function(pm):
    text = open(os.path.join(ROOT, "include", "pm", "imaging.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = pm.load()
    assert re.search(r"\bint\s+pm_fuse_disparity\s*\(\s*pm_handle\s*\*", text) and "typedef struct pm_fuse_options" in text
    assert text.index("pm_disparity_confidence") < text.index("pm_fuse_disparity")
    assert "pm_fuse_disparity" in pm.EXPORTS and hasattr(lib, "pm_fuse_disparity")
    assert C.sizeof(pm.PmFuseOptions) == 24
    assert (pm.PM_FUSE_VALID, pm.PM_FUSE_KEPT, pm.PM_FUSE_FUSED, pm.PM_FUSE_FILLED) == (FU.VALID, FU.KEPT, FU.FUSED, FU.FILLED)
    assert re.search(r"PM_FUSE_VALID\s*=\s*1\s*,\s*PM_FUSE_KEPT\s*=\s*2\s*,\s*PM_FUSE_FUSED\s*=\s*4\s*,\s*PM_FUSE_FILLED\s*=\s*8", text)
    csrc = os.path.join(ROOT, "ocean-perception_amd", "csrc")
    assert '#include "pm_fuse.hpp"' in open(os.path.join(csrc, "pm_stages.hip")).read()  # the kernels live in that unit alone
    for f in os.listdir(csrc):
        if f.endswith(".hip") and f != "pm_stages.hip":
            assert "pm_fuse" not in open(os.path.join(csrc, f)).read(), f


# ---- 3. device parity ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        yield e


def _check(torch, engine, shape, names, radius=0, fill=None, weighted=False, **kw):
    rows, cols = SHAPES[shape]
    cur, cam, sources, mots, _ = fuse_case(rows, cols, names, very_near="behind" in names)
    n = len(names)
    w, ws = _weights(rows, cols, n) if weighted else (None, None)
    return FF.check_fuse(torch, engine, cur, list(sources), cam, list(mots), w, None if ws is None else list(ws),
                         **dict(OPT, radius=radius), fill_min_sources=min(2, n) if fill is None else fill,
                         want=_want(shape, names, radius, fill, weighted), **kw)


@gpu
@pytest.mark.parametrize("motion", REAL + ("behind", "gone"))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fuse_equals_the_definition(pm, engine, shape, motion):
    """Six shapes (one pixel, a row shorter than a wavefront, rows that are no multiple of the block's 4, a row that crosses
    the 256-pixel span with a ragged tail, several blocks both ways) x seven motions x n = 1, 3: the four maps, d_counts and
    the host counts at tolerance 0, with the fill and, for n = 3, with weights too."""
    import torch
    _check(torch, engine, shape, _names(motion, 1))
    _check(torch, engine, shape, _names(motion, 3))
    _check(torch, engine, shape, _names(motion, 3), radius=1, weighted=True)


@gpu
@pytest.mark.parametrize("shape", ["37x53", "64x96"])
def test_eight_sources(pm, engine, shape):
    import torch
    want = _check(torch, engine, shape, _names("yaw", 8), radius=1, weighted=True)
    assert want["count"].max() >= 7 and want["counts"][3] > 0


@gpu
@pytest.mark.parametrize("radius", [0, 1, 2])
def test_every_radius(pm, engine, radius):
    import torch
    _check(torch, engine, "37x53", THREE, radius=radius)


@gpu
@pytest.mark.parametrize("fill", [0, 1, 2])
def test_every_fill_min_sources(pm, engine, fill):
    import torch
    want = _check(torch, engine, "37x53", THREE, fill=fill)
    assert (want["counts"][3] > 0) == (fill > 0)
    assert fill == 0 or want["counts"][3] <= _want("37x53", THREE, 0, 1)["counts"][3]


@gpu
def test_each_output_alone_in_place_and_unaligned(pm, engine):
    """Every output asked for alone; d_out == d_disp; base pointers 4, 8 and 12 bytes past a 16-byte boundary (1, 2 and 3 for
    the byte maps); the weights all null as a null array and as an array of nulls."""
    import torch
    for only in FF.OUTPUTS:
        _check(torch, engine, "17x131", THREE, radius=1, weighted=True, outputs=(only,))
    _check(torch, engine, "17x131", THREE, radius=1, weighted=True, in_place=True)
    _check(torch, engine, "9x300", THREE, outputs=("out",), in_place=True)
    for off in (1, 2, 3):
        _check(torch, engine, "9x300", THREE, radius=1, weighted=True, offset_floats=off)
    _check(torch, engine, "37x53", THREE, array_of_nulls=True)


@gpu
def test_special_values_in_maps_and_weights_and_a_source_that_is_the_map(pm, engine):
    """NaN, -0.0, negatives, +inf and subnormals in the current map and in the sources; NaN, -1, 0 and +-inf in the weight
    planes; some weight entries null; the current map's own buffer as a source."""
    import torch
    rows, cols = 37, 53
    rng = np.random.default_rng(9)
    cur, cam, sources, mots, _ = fuse_case(rows, cols, ("yaw", "identity", "baseline"))
    cur, sources = cur.copy(), [s.copy() for s in sources]
    for a in [cur] + sources:
        pick = rng.random((rows, cols)) < 0.1
        a[pick] = rng.choice(FF.SPECIALS, int(pick.sum()))
    cur.ravel()[:FF.SPECIALS.size] = FF.SPECIALS
    w = FF.random_weight(rng, rows, cols, special=0.5)
    ws = [FF.random_weight(rng, rows, cols, special=0.5), None, FF.random_weight(rng, rows, cols, special=0.5)]
    for radius in (0, 2):
        want = FF.check_fuse(torch, engine, cur, sources, cam, list(mots), w, ws, **dict(OPT, radius=radius, max_conflicts=1),
                             fill_min_sources=1)
        assert 0 < want["counts"][2] < want["counts"][1] < want["counts"][0] and want["counts"][3] > 0
        assert np.isinf(want["out"]).any() or np.isnan(want["spread"]).any()
    inf = np.full((rows, cols), np.inf, np.float32)
    want = FF.check_fuse(torch, engine, inf, [inf], cam, [IDENT], max_diff=1.0, radius=0, min_consistent=0, max_conflicts=8)
    assert (FF.bits(want["spread"]) == 0x7FC00000).all()
    FF.check_fuse(torch, engine, cur, [cur, sources[0]], cam, [IDENT, mots[0]], None, [ws[0], None], max_diff=0.0, radius=1,
                  min_consistent=1, max_conflicts=0, fill_min_sources=2, self_source=(0,))


@gpu
def test_kept_pixels_are_the_consistency_filters(pm, engine):
    """With null weights and the fill off, the zero set of d_out and counts[0..1] are pm_filter_consistency's on the same device
    buffers."""
    import torch
    cur, cam, sources, mots, _ = fuse_case(64, 96, REAL)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d, src = up(cur), [up(s) for s in sources]
    a, b = torch.zeros_like(d), torch.zeros_like(d)
    torch.cuda.synchronize()
    ptrs = [s.data_ptr() for s in src]
    for radius, mc, mx in ((0, 2, 0), (1, 3, 1), (2, 5, 0)):
        n_f = engine.fuse_disparity(cam, d.data_ptr(), ptrs, list(mots), 64, 96, MAX_DIFF, radius, mc, mx, d_out=a.data_ptr(), want_counts=True)
        n_c = engine.filter_consistency(cam, d.data_ptr(), ptrs, list(mots), 64, 96, MAX_DIFF, radius, mc, mx, d_out=b.data_ptr(), want_counts=True)
        engine.synchronize()
        assert tuple(n_f[:2]) == tuple(n_c) and 0 < n_c[1] < n_c[0] and n_f[3] == 0
        assert np.array_equal(a.cpu().numpy() == 0, b.cpu().numpy() == 0)


@gpu
def test_invalid_arguments_are_named_and_nothing_is_enqueued(pm, engine):
    """PM_ERR_INVALID_ARG with pm_last_error naming the argument; every output keeps its guard pattern."""
    import torch
    rows, cols = 16, 24
    lib, h = engine.lib, engine.h
    disp = torch.full((rows, cols), 10.0, dtype=torch.float32, device="cuda")
    other = torch.full((2, rows, cols), 10.0, dtype=torch.float32, device="cuda")
    wts = torch.full((2, rows, cols), 1.0, dtype=torch.float32, device="cuda")
    px = rows * cols
    outs = {k: FF.Guarded(torch, n) for k, n in (("out", 4 * px), ("cnt", px), ("spr", 4 * px), ("flg", px), ("c", 16))}
    good = camera_for(rows, cols)
    host = (C.c_int * 4)(-5, -5, -5, -5)
    UNSET = object()
    two = [other[0].data_ptr(), other[1].data_ptr()]

    def call(cam=good, opt=(1.0, 1, 1, 0, 1, 0.5), d=UNSET, src=two, n=None, mot=UNSET, w=None, shape=(rows, cols), out=UNSET,
             cnt=UNSET, spr=UNSET, flg=UNSET, c=UNSET, hc=host):
        cc = pm.cloud_camera(cam)
        o = pm.PmFuseOptions(*opt) if opt is not None else None
        pick = lambda v, default: default if v is UNSET else v
        arr = (C.c_void_p * len(src))(*src) if src is not None else None
        warr = (C.c_void_p * len(w))(*w) if w is not None else None
        count = len(src) if n is None else n
        mots = pick(mot, [FF.IDENTITY] * (len(src) if src is not None else 1))
        m = (pm.PmMotion * len(mots))(*[pm.as_motion(v) for v in mots]) if mots is not None else None
        return lib.pm_fuse_disparity(h, C.byref(cc) if cc is not None else None, C.byref(o) if o is not None else None,
                                     pick(d, disp.data_ptr()), None, count, arr, m, warr, shape[0], shape[1],
                                     pick(out, outs["out"].ptr), pick(cnt, outs["cnt"].ptr), pick(spr, outs["spr"].ptr),
                                     pick(flg, outs["flg"].ptr), pick(c, outs["c"].ptr), hc)

    def refused(rc, word, status=pm.PM_ERR_INVALID_ARG):
        text = lib.pm_last_error(h).decode()
        assert rc == status and word in text and "pm_fuse_disparity" in text, (rc, word, text)

    refused(call(cam=None), "camera")
    refused(call(opt=None), "options")
    refused(call(d=None), "d_disp")
    refused(call(src=None, n=2, mot=[FF.IDENTITY] * 2), "d_sources")
    refused(call(mot=None), "motions")
    refused(call(src=[two[0], None]), "d_sources[1]")
    for i, name in enumerate(("fx", "fy", "cx", "cy", "baseline")):
        for bad in (np.nan, np.inf, -np.inf):
            cam = list(good)
            cam[i] = bad
            refused(call(cam=cam), name)
    refused(call(cam=(0.0,) + good[1:]), "fx")
    refused(call(cam=(good[0], 0.0) + good[2:]), "fy")
    refused(call(src=[], n=0, mot=[FF.IDENTITY]), "n_sources")
    refused(call(src=two * 4 + two[:1], mot=[FF.IDENTITY] * 9), "n_sources")
    refused(call(n=-1), "n_sources")
    for i in range(12):
        for bad in (np.nan, np.inf, -np.inf):
            R, t = np.eye(3).ravel(), np.zeros(3)
            (R if i < 9 else t)[i if i < 9 else i - 9] = bad
            refused(call(mot=[FF.IDENTITY, (R, t)]), ("R[%d]" % i if i < 9 else "t[%d]" % (i - 9)) + " of motions[1]")
    for bad in (np.nan, np.inf, -0.5):
        refused(call(opt=(bad, 1, 1, 0, 1, 0.5)), "max_diff")
        refused(call(opt=(1.0, 1, 1, 0, 1, bad)), "fill_max_diff")
    refused(call(opt=(1.0, 1, 1, 0, 0, np.nan)), "fill_max_diff")  # also where nothing would be filled
    refused(call(opt=(1.0, -1, 1, 0, 1, 0.5)), "radius")
    refused(call(opt=(1.0, 3, 1, 0, 1, 0.5)), "radius")
    refused(call(opt=(1.0, 1, -1, 0, 1, 0.5)), "min_consistent")
    refused(call(opt=(1.0, 1, 3, 0, 1, 0.5)), "min_consistent")
    refused(call(opt=(1.0, 1, 1, -1, 1, 0.5)), "max_conflicts")
    refused(call(opt=(1.0, 1, 1, 9, 1, 0.5)), "max_conflicts")
    refused(call(opt=(1.0, 1, 1, 0, -1, 0.5)), "fill_min_sources")
    refused(call(opt=(1.0, 1, 1, 0, 3, 0.5)), "fill_min_sources")
    refused(call(shape=(0, cols)), "empty")
    refused(call(shape=(rows, 0)), "empty")
    refused(call(shape=(rows, -3)), "empty")
    refused(call(out=None, cnt=None, spr=None, flg=None, c=None, hc=None), "no output")
    for name, key in (("d_out", "out"), ("d_count", "cnt"), ("d_spread", "spr"), ("d_flags", "flg")):
        refused(call(**{key: two[1]}), name + " must not alias d_sources[1]")
        refused(call(w=[None, wts[1].data_ptr()], **{key: wts[1].data_ptr()}), name + " must not alias d_source_weights[1]")
    refused(call(src=[two[0], disp.data_ptr()], out=disp.data_ptr()), "d_sources[1]")  # in place on a map that is a source
    refused(call(shape=(70000, 40000)), "exceed", pm.PM_ERR_SIZE)
    engine.synchronize()
    for buf in outs.values():
        buf.read(np.uint8, 0)
    assert tuple(host) == (-5,) * 4 and (disp.cpu().numpy() == 10.0).all() and (other.cpu().numpy() == 10.0).all()
    # and the same arguments made good do run
    assert call() == pm.PM_OK and tuple(host) == (px, px, px, 0)
    assert call(src=[two[0], disp.data_ptr()], w=[wts[0].data_ptr(), None]) == pm.PM_OK  # a source may be the current map


@gpu
def test_fuse_scratch_is_owned_by_the_handle(pm):
    """The four counts and, for a call that fills, the n splat maps are ONE handle-owned allocation through csrc/pm_devbuf.hpp:
    16 bytes on first use without a fill, grown for a fill and for more sources or pixels, reused below that, gone with the
    handle."""
    import torch
    lib = pm.load()
    live = lambda: (lib.pm_debug_live_device_allocations(), lib.pm_debug_live_device_bytes())
    before = live()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        base = live()
        small = torch.full((37, 53), 3.0, dtype=torch.float32, device="cuda")
        large = torch.full((300, 500), 3.0, dtype=torch.float32, device="cuda")
        small[5, 7], large[5, 7] = 0.0, 0.0
        flg = torch.zeros((300, 500), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        run = lambda t, n, fill: e.fuse_disparity(camera_for(*t.shape), t.data_ptr(), [t.data_ptr()] * n, [FF.IDENTITY] * n,
                                                  t.shape[0], t.shape[1], fill_min_sources=fill, d_flags=flg.data_ptr(),
                                                  want_counts=True)
        px = 37 * 53
        assert run(small, 1, 0) == (px - 1, px - 1, px - 1, 0)
        assert live() == (base[0] + 1, base[1] + 16)
        assert run(large, 8, 0) == (150000 - 1,) * 3 + (0,) and live() == (base[0] + 1, base[1] + 16)
        assert run(small, 3, 1)[3] == 0  # the sources are the map itself: nothing lands on its hole
        grown = live()
        assert grown == (base[0] + 1, base[1] + 16 + 3 * 4 * px)
        assert run(small, 2, 2) == (px - 1, px - 1, px - 1, 0) and live() == grown
        run(large, 2, 1)
        assert live() == (base[0] + 1, base[1] + 16 + 2 * 4 * 150000)
    assert live() == before


# ---- 4. through a sequence: three matches, the newest fused against the other two -------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["scalar", "planes"])
def test_the_newest_map_is_fused_against_two_earlier_matches_on_the_handles_stream(pm, synth, mode):
    """Three Matches of synthetic pairs on ONE handle into three buffers, then the newest left map fused against the other two
    on the handle's stream, nothing copied and nothing synchronised in between: the result equals the definition on the
    downloaded maps."""
    import torch
    rows, cols = 96, 128
    cam = camera_for(rows, cols)
    kw = dict(mode=pm.PM_MODE_PLANES) if mode == "planes" else {}
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    pairs = [synth.make_pair(3 + k, rows=rows, cols=cols, n_points=40, dilate_factor=2) for k in range(3)]
    dev = [[up(p[k]) for k in ("left", "right", "seed_l", "seed_r")] for p in pairs]
    D = torch.zeros((3, 2, rows, cols), dtype=torch.float32, device="cuda")
    out = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    spr = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((rows, cols), dtype=torch.uint8, device="cuda")
    flg = torch.zeros((rows, cols), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    mots = [FF.IDENTITY, (FF.rotation((0, 1, 0), 0.5).ravel(), np.array([0.01, 0.0, 0.0]))]
    opt = dict(max_diff=1.0, radius=1, min_consistent=0, max_conflicts=1, fill_min_sources=1, fill_max_diff=1.0)
    with pm.Engine(pm.default_params(0, patch=5, patchmatch_iters=2, max_disp=32, **kw), max_rows=rows, max_cols=cols) as e:
        for k, (L, R, SL, SR) in enumerate(dev):
            e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), D[k, 0].data_ptr(), D[k, 1].data_ptr())
        n = e.fuse_disparity(cam, D[2, 0].data_ptr(), [D[1, 0].data_ptr(), D[0, 0].data_ptr()], mots, rows, cols, d_out=out.data_ptr(),
                             d_count=cnt.data_ptr(), d_spread=spr.data_ptr(), d_flags=flg.data_ptr(), want_counts=True, **opt)
        e.synchronize()
    maps = D.cpu().numpy()
    assert not np.array_equal(maps[0, 0], maps[1, 0]) and not np.array_equal(maps[1, 0], maps[2, 0])
    want = FU.fuse(maps[2, 0], [maps[1, 0], maps[0, 0]], cam, mots, **opt)
    print(mode, "valid, kept, fused, filled:", want["counts"])
    assert want["counts"][0] > 0.25 * rows * cols and want["counts"][2] > 0 and want["counts"][3] > 0
    assert n == tuple(int(v) for v in want["counts"])
    assert np.array_equal(FF.bits(out.cpu().numpy()), FF.bits(want["out"]))
    assert np.array_equal(cnt.cpu().numpy(), want["count"]) and np.array_equal(flg.cpu().numpy(), want["flags"])
    assert np.array_equal(FF.bits(spr.cpu().numpy()), FF.bits(want["spread"]))


@gpu
def test_fuzz_fuse_one_short_seeded_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_fuse.py"), "--cases", "20", "--seed", "4"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
