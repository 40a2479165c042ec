"""Geometric consistency: the current left map judged by earlier maps of its sequence (include/pm/imaging.h:
pm_filter_consistency).

CPU tests pin the definition (tests/consistency_ref.py) against analytic cases and run the kernel's own per-thread code
(csrc/pm_consistency_body.hpp) on the host under ASan / UBSan, blocks forwards and backwards.  GPU tests hold the kernel to the
definition with tolerance 0 -- every operation of the definition is one IEEE rounding, the build uses -ffp-contract=off, and
only integer addition crosses workgroups -- with guard bands around every output.  Every case is first shown to be non-trivial
ON THE DEFINITION ALONE: all four classes populated, a keep rule that keeps most and removes some."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import consistency_ref as CR
import reproject_ref as RR
from conftest import ROOT
from cpp_build import build_host_kernel
from host_run import assert_program_compares, dump_case, flat_motions
from pointcloud_ref import camera_for
from test_reproject import CAM, FXB, motions, two_level

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_consistency as FC  # noqa: E402  (check_consistency: the device-against-definition comparison)

gpu = pytest.mark.gpu

I3 = np.eye(3).ravel()
ZERO = np.zeros(3)
SHAPES = {"1x1": (1, 1), "1x7": (1, 7), "37x53": (37, 53), "64x96": (64, 96), "17x131": (17, 131), "9x300": (9, 300)}
REAL = ("identity", "baseline", "advance", "yaw", "roll")  # the motions that leave something to see
MAX_DIFF = 0.75  # above the +-0.3 of a disturbed source and the +-0.2 relief of a neighbouring pixel, below the steps of 4


# ---- 1. the definition ------------------------------------------------------------------------------------------------
def test_definition_identity_against_itself_keeps_the_map_bit_for_bit():
    """20 random 48x80 maps, 20 % zeros, d in 0.01 .. 128: R = I, t = 0 and the map as its own source land every pixel on
    itself, so with max_diff = 0 every valid pixel is CONSISTENT, the residual is +0.0 and d_out is the map."""
    rng = np.random.default_rng(11)
    for _ in range(20):
        d = rng.uniform(0.01, 128.0, (48, 80)).astype(np.float32)
        d[rng.random((48, 80)) < 0.2] = 0.0
        for r in (0, 1):
            out = CR.filter_consistency(d, [d], CAM, [(I3, ZERO)], max_diff=0.0, radius=r, min_consistent=1, max_conflicts=0)
            assert np.array_equal(out["per_source"][0], np.where(d > 0, CR.CONSISTENT, CR.UNSEEN))
            assert np.array_equal(FC.bits(out["out"]), FC.bits(d)) and not FC.bits(out["residual"]).any()
            assert tuple(out["counts"]) == ((d > 0).sum(), (d > 0).sum())


def test_definition_projection_is_the_reproject_splat():
    """The projection is pm_reproject_disparity's: raised to the maximum per target, it IS reproject_ref's left splat."""
    d = two_level(37, 53, seed=2)
    cam = camera_for(37, 53)
    for name, (R, t) in motions(cam, FXB / 6.0).items():
        seen, iu, iv, dp = CR.project(d, cam, R, t)
        want, hits = RR.splat_left(d, cam, R, t)
        got = RR._raise_to_max(37, 53, seen, iv, iu, dp)
        assert np.array_equal(FC.bits(got[0]), FC.bits(want)) and np.array_equal(got[1], hits), name
        assert seen.any() == (name != "gone")


def test_definition_occluded_and_conflict_boxes():
    d = np.random.default_rng(3).uniform(8.0, 12.0, (48, 80)).astype(np.float32)
    box = np.zeros((48, 80), bool)
    box[10:20, 30:50] = True
    near = d.copy()
    near[box] += np.float32(4)
    out = CR.filter_consistency(d, [near], CAM, [(I3, ZERO)], max_diff=1.0, radius=0)
    assert np.array_equal(out["per_source"][0], np.where(box, CR.OCCLUDED, CR.CONSISTENT))
    assert out["kept"].sum() == (~box).sum()  # an occluded pixel has nobody who confirms it
    through = d.copy()
    through[box] = np.float32(2)
    out = CR.filter_consistency(d, [through], CAM, [(I3, ZERO)], max_diff=1.0, radius=0)
    assert np.array_equal(out["per_source"][0], np.where(box, CR.CONFLICT, CR.CONSISTENT))
    assert np.array_equal(out["out"], np.where(box, np.float32(0), d)) and tuple(out["counts"]) == (48 * 80, (~box).sum())


def test_definition_baseline_shift_and_advance():
    d = np.full((48, 80), 20.0, np.float32)
    # the source camera where the current right camera is: a constant-20 map moves by 20 columns
    out = CR.filter_consistency(d, [d], CAM, [(I3, (-0.12, 0.0, 0.0))], max_diff=0.0, radius=0)
    assert (out["per_source"][0][:, :20] == CR.UNSEEN).all() and (out["per_source"][0][:, 20:] == CR.CONSISTENT).all()
    assert tuple(out["counts"]) == (48 * 80, 48 * 60) and not FC.bits(out["residual"]).any()
    # an advance by 10 % of the range towards a constant plane: the disparity grows to d0 / 0.9
    t = (0.0, 0.0, -0.1 * (FXB / 20.0))
    src = np.full((48, 80), np.float32(20.0 / 0.9), np.float32)
    out = CR.filter_consistency(d, [src], CAM, [(I3, t)], max_diff=1e-5, radius=0)
    seen = CR.project(d, CAM, I3, t)[0]
    assert 0.5 < seen.mean() < 1.0  # the image spreads about the principal point: its rim leaves
    assert np.array_equal(out["per_source"][0], np.where(seen, CR.CONSISTENT, CR.UNSEEN))
    assert out["residual"].max() <= 4e-6


def test_definition_tap_rule_the_first_of_two_equal_wins():
    d = np.full((7, 9), 10.0, np.float32)
    at = lambda taps, r, **kw: CR.filter_consistency(d, [taps], camera_for(7, 9), [(I3, ZERO)], max_diff=0.5, radius=r, **kw)
    s = np.zeros((7, 9), np.float32)
    s[2, 3], s[4, 5] = 11.0, 9.0  # (dy, dx) = (-1, -1): e = +1 comes first; (1, 1): e = -1
    out = at(s, 1)
    assert out["per_source"][0][3, 4] == CR.OCCLUDED
    s[2, 3], s[4, 5] = 9.0, 11.0
    assert at(s, 1)["per_source"][0][3, 4] == CR.CONFLICT
    assert at(s, 0)["per_source"][0][3, 4] == CR.UNSEEN  # the centre itself has no value
    s[4, 4] = 10.25  # later, but strictly smaller: it replaces
    out = at(s, 1)
    assert out["per_source"][0][3, 4] == CR.CONSISTENT and out["residual"][3, 4] == np.float32(0.25)
    s = np.zeros((7, 9), np.float32)
    s[1, 6], s[4, 2] = 9.0, 11.0  # (-2, 2): e = -1 comes first; (1, -2): e = +1
    assert at(s, 2)["per_source"][0][3, 4] == CR.CONFLICT and at(s, 1)["per_source"][0][3, 4] == CR.UNSEEN
    s[1, 6], s[4, 2] = 11.0, 9.0
    assert at(s, 2)["per_source"][0][3, 4] == CR.OCCLUDED
    s[1, 6] = np.inf  # e = +inf is first and loses against the finite one behind it
    assert at(s, 2)["per_source"][0][3, 4] == CR.CONFLICT
    s[4, 2] = 0.0  # alone, +inf is something nearer
    assert at(s, 2)["per_source"][0][3, 4] == CR.OCCLUDED
    # taps outside the image do not count: the corner pixel sees its own 2 x 2 (radius 1) only
    s = np.zeros((7, 9), np.float32)
    s[1, 1] = 10.0
    out = at(s, 1)
    assert out["per_source"][0][0, 0] == CR.CONSISTENT and out["per_source"][0][0, 3] == CR.UNSEEN


def test_definition_special_values_in_the_map_and_in_a_source():
    cam = camera_for(16, 24)
    d = np.full((16, 24), 9.0, np.float32)
    d.ravel()[:FC.SPECIALS.size] = FC.SPECIALS  # 0, -0.0, -1, -37.5, NaN, +inf, three subnormal / tiny values
    out = CR.filter_consistency(d, [d], cam, [(I3, ZERO)], max_diff=0.0, radius=0)
    with np.errstate(invalid="ignore"):
        valid = d > 0
    assert valid.ravel()[:9].tolist() == [False] * 5 + [True] * 4 and out["counts"][0] == valid.sum()
    assert not out["classes"].ravel()[:5].any() and not FC.bits(out["residual"]).ravel()[:5].any()
    assert out["classes"].ravel()[5] == CR.UNSEEN  # +inf: a point at range 0 is in front of no camera
    assert np.array_equal(FC.bits(out["out"]).ravel()[:5], FC.bits(d).ravel()[:5])  # invalid pixels keep their bits
    assert FC.bits(out["out"]).ravel()[5] == 0  # valid, confirmed by nobody: +0.0
    s = np.full((16, 24), 9.0, np.float32)
    s.ravel()[:6] = FC.SPECIALS[:6]
    full = np.full((16, 24), 9.0, np.float32)
    out = CR.filter_consistency(full, [s], cam, [(I3, ZERO)], max_diff=0.0, radius=0)
    assert out["per_source"][0].ravel()[:6].tolist() == [CR.UNSEEN] * 5 + [CR.OCCLUDED]
    assert (out["per_source"][0].ravel()[6:] == CR.CONSISTENT).all()


def _eight_sources(d):
    """Sources 0..7 with the classes 0, 1, 2, 3, 0, 1, 2, 3 at every pixel."""
    kinds = [np.zeros_like(d), d, d + np.float32(4), np.full_like(d, 2.0)]
    return [kinds[k % 4] for k in range(8)], [(I3, ZERO)] * 8


def test_definition_keep_rule_and_the_bit_layout_of_eight_sources():
    d = np.random.default_rng(5).uniform(8.0, 12.0, (9, 13)).astype(np.float32)
    d[2, 3] = 0.0
    sources, mots = _eight_sources(d)
    out = CR.filter_consistency(d, sources, CAM, mots, max_diff=1.0, radius=0, min_consistent=2, max_conflicts=2)
    word = sum((k % 4) << (2 * k) for k in range(8))
    assert word == 0xE4E4 and (out["classes"][d > 0] == word).all() and out["classes"][2, 3] == 0
    assert out["classes"].dtype == np.uint16 and out["kept"].sum() == d.size - 1
    keeps = lambda **kw: int(CR.filter_consistency(d, sources, CAM, mots, max_diff=1.0, radius=0, **kw)["counts"][1])
    n = d.size - 1
    assert keeps(min_consistent=0, max_conflicts=8) == n and keeps(min_consistent=0, max_conflicts=2) == n
    assert keeps(min_consistent=0, max_conflicts=0) == 0 and keeps(min_consistent=0, max_conflicts=1) == 0
    assert keeps(min_consistent=8, max_conflicts=8) == 0 and keeps(min_consistent=3, max_conflicts=8) == 0
    assert keeps(min_consistent=2, max_conflicts=8) == n
    one = CR.filter_consistency(d, [d], CAM, [(I3, ZERO)], max_diff=0.0, radius=0, min_consistent=1, max_conflicts=0)
    assert one["counts"][1] == n  # n = 1: min_consistent = n


# ---- the cases the kernel is held to, and what makes them worth running ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(shape, motion, n):
    """The current map (two_level), and n sources: the first under `motion`, the others under the real motions in turn; each
    the map carried into its view and disturbed (tools/fuzz_consistency.py: disturbed_source)."""
    rows, cols = SHAPES[shape]
    cam = camera_for(rows, cols)
    cur = two_level(rows, cols, seed=rows + cols, very_near=motion == "behind")
    table = motions(cam, FXB / 6.0)
    first = REAL.index(motion) + 1 if motion in REAL else 0
    names = [motion] + [REAL[(first + j) % len(REAL)] for j in range(n - 1)]
    mots = [table[name] for name in names]
    sources = [FC.disturbed_source(cur, cam, m, seed=100 * k + rows + cols) for k, m in enumerate(mots)]
    return cur, cam, sources, mots


@functools.lru_cache(maxsize=None)
def _want(shape, motion, n, radius):
    cur, cam, sources, mots = _case(shape, motion, n)
    return CR.filter_consistency(cur, sources, cam, mots, MAX_DIFF, radius, min(2, n), 0)


def test_conditions_every_class_is_populated():
    """On 37x53 and 64x96, radius 0, one source, the five real motions: each class holds at least 0.5 % of the valid pixels."""
    for shape in ("37x53", "64x96"):
        for motion in REAL:
            want = _want(shape, motion, 1, 0)
            share = np.bincount(want["per_source"][0][want["valid"]], minlength=4) / want["valid"].sum()
            print(shape, motion, "shares of UNSEEN / CONSISTENT / OCCLUDED / CONFLICT:", share.round(4))
            assert (share >= 0.005).all(), (shape, motion, share)


def test_conditions_the_keep_rule_keeps_most_and_removes_some():
    """Three sources identity / baseline / yaw, max_diff 0.75, min_consistent 2, max_conflicts 0: 50 % .. 97 % are kept."""
    for shape in ("37x53", "64x96"):
        cur, cam, _, _ = _case(shape, "identity", 1)
        table = motions(cam, FXB / 6.0)
        mots = [table[name] for name in ("identity", "baseline", "yaw")]
        sources = [FC.disturbed_source(cur, cam, m, seed=7 + k) for k, m in enumerate(mots)]
        want = CR.filter_consistency(cur, sources, cam, mots, 0.75, 0, 2, 0)
        share = want["counts"][1] / want["counts"][0]
        print(shape, "kept share:", share)
        assert 0.50 <= share <= 0.97, (shape, share)


def test_conditions_thin_shapes_keep_and_remove():
    """On the thin shapes, radius 0: at least one pixel is kept and at least one is removed -- under every real motion where
    the shape has room for the boxes (17x131, 9x300), and over the real motions together where rows / 6 is 0 and only the
    motion and the zeroed 5 % remove anything (1x7; 1x1, whose one pixel is kept under one motion and lost under another)."""
    for shape in ("17x131", "9x300"):
        for motion in REAL:
            v, k = _want(shape, motion, 1, 0)["counts"]
            print(shape, motion, "valid", v, "kept", k)
            assert 1 <= k < v, (shape, motion, v, k)
    for shape in ("1x7", "1x1"):
        counts = [tuple(int(c) for c in _want(shape, motion, 1, 0)["counts"]) for motion in REAL]
        print(shape, "(valid, kept) under", REAL, counts)
        assert any(k >= 1 for v, k in counts) and any(k < v for v, k in counts), (shape, counts)


def test_conditions_behind_and_gone_leave_nothing_to_see():
    for shape in ("37x53", "64x96", "17x131", "9x300"):
        cur, cam, sources, mots = _case(shape, "behind", 1)
        assert (cur == 200.0).sum() > 20 and (_want(shape, "behind", 1, 2)["per_source"][0][cur == 200.0] == CR.UNSEEN).all()
        assert not _want(shape, "gone", 1, 2)["per_source"][0].any() and _want(shape, "gone", 1, 2)["counts"][1] == 0
        assert _want(shape, "gone", 3, 0)["counts"][1] > 0  # the other two sources still confirm


# ---- 2. the kernel's own per-thread code, run on the host ------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_consistency_exe(tmp_path_factory):
    """tests/cpp/consistency_host_main.cpp: csrc/pm_consistency_body.hpp compiled for the host alone, with the sanitizers."""
    return build_host_kernel(tmp_path_factory.mktemp("consistencyhost") / "consistency_host_main", "consistency_host_main.cpp")


def _dump_case(path, cur, cam, sources, mots, max_diff, radius, min_consistent, max_conflicts):
    want = CR.filter_consistency(cur, sources, cam, mots, max_diff, radius, min_consistent, max_conflicts)
    dump_case(path, [*cur.shape, *cam, len(sources), radius, max_diff, min_consistent, max_conflicts, *flat_motions(mots, CR.MAX_SOURCES)],
              disp=cur, sources=np.stack(sources).astype(np.float32), want_out=want["out"], want_classes=want["classes"],
              want_residual=want["residual"], want_counts=want["counts"])
    return want


def test_kernel_code_on_the_host_equals_the_definition(host_consistency_exe, tmp_path):
    """Every thread of the launch over whole maps on the CPU, forwards, backwards, in place and with the counts alone: all four
    outputs equal the .npy dumps of the definition byte for byte, and AddressSanitizer / UBSan see every access into buffers of
    exactly the size the stage may touch.  Six shapes x n = 1, 3, 8 x radius 0..2, the motions in turn, special values in
    the current map and in the sources."""
    names = REAL + ("behind", "gone")
    kept, k = 0, 0
    for shape in SHAPES:
        for n in (1, 3, 8):
            for radius in (0, 1, 2):
                cur, cam, sources, mots = _case(shape, names[k % len(names)], n)
                cur, sources = cur.copy(), [s.copy() for s in sources]
                m = min(FC.SPECIALS.size, cur.size - 1)
                cur.ravel()[:m] = FC.SPECIALS[:m]
                sources[-1].ravel()[cur.size - m:] = FC.SPECIALS[:m]
                d = str(tmp_path / ("case%d" % k))
                kept += int(_dump_case(d, cur, cam, sources, mots, MAX_DIFF, radius, min(2, n), k % 2)["counts"][1])
                r = subprocess.run([host_consistency_exe, d], capture_output=True, text=True)
                assert r.returncode == 0, (shape, n, radius, r.stderr[-3000:])
                k += 1
    assert kept > 10000
    # the program does compare: one flipped bit in an expectation is a mismatch, not a pass
    assert_program_compares(host_consistency_exe, str(tmp_path / "case30"),
                            [("want_residual", np.uint32, "residual differs"), ("want_classes", np.uint16, "classes differs"),
                             ("want_out", np.uint32, "out differs"), ("want_counts", np.int32, "counts differs")])


def test_headers_declare_and_the_library_exports_the_consistency_function(pm):
    text = open(os.path.join(ROOT, "include", "pm", "imaging.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = pm.load()
    assert re.search(r"\bint\s+pm_filter_consistency\s*\(\s*pm_handle\s*\*", text)
    assert "typedef struct pm_consistency_options" in text and re.search(r"#define\s+PM_CONSISTENCY_MAX_SOURCES\s+8\b", text)
    assert "pm_filter_consistency" in pm.EXPORTS and hasattr(lib, "pm_filter_consistency")
    assert C.sizeof(pm.PmConsistencyOptions) == 16 and pm.PM_CONSISTENCY_MAX_SOURCES == CR.MAX_SOURCES == 8
    assert (pm.PM_CONSISTENCY_UNSEEN, pm.PM_CONSISTENCY_CONSISTENT, pm.PM_CONSISTENCY_OCCLUDED, pm.PM_CONSISTENCY_CONFLICT) == (
        CR.UNSEEN, CR.CONSISTENT, CR.OCCLUDED, CR.CONFLICT)
    stages = open(os.path.join(ROOT, "ocean-perception_amd", "csrc", "pm_stages.hip")).read()
    assert '#include "pm_consistency.hpp"' in stages  # the kernels live in that unit alone
    for f in os.listdir(os.path.join(ROOT, "ocean-perception_amd", "csrc")):
        if f.endswith(".hip") and f != "pm_stages.hip":
            assert "pm_consistency" not in open(os.path.join(ROOT, "ocean-perception_amd", "csrc", f)).read(), f


# ---- 3. device parity ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        yield e


@gpu
@pytest.mark.parametrize("motion", REAL + ("behind", "gone"))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_consistency_equals_the_definition(pm, engine, shape, motion):
    """Six shapes (one pixel, a row shorter than a wavefront, rows that are no multiple of the block's 4, a row that crosses
    the 256-pixel span with a ragged tail, several blocks both ways) x seven motions x n = 1, 3, 8 x radius 0, 1, 2: the three
    maps, d_counts and the host counts at tolerance 0; then every output alone and d_out == d_disp."""
    import torch
    for n in (1, 3, 8):
        cur, cam, sources, mots = _case(shape, motion, n)
        for radius in (0, 1, 2):
            FC.check_consistency(torch, engine, cur, sources, cam, mots, MAX_DIFF, radius, min(2, n), 0,
                                 want=_want(shape, motion, n, radius))
    cur, cam, sources, mots = _case(shape, motion, 3)
    want = _want(shape, motion, 3, 1)
    for only in FC.OUTPUTS:
        FC.check_consistency(torch, engine, cur, sources, cam, mots, MAX_DIFF, 1, 2, 0, outputs=(only,), want=want)
    FC.check_consistency(torch, engine, cur, sources, cam, mots, MAX_DIFF, 1, 2, 0, in_place=True, want=want)
    FC.check_consistency(torch, engine, cur, sources, cam, mots, MAX_DIFF, 1, 2, 0, outputs=("out",), in_place=True, want=want)


@gpu
def test_special_values_eight_sources_and_a_source_that_is_the_map(pm, engine):
    """Special values in the current map and in the sources; the eight-source bit layout; the keep rule at its ends; the
    current map's own buffer as a source."""
    import torch
    rows, cols = 37, 53
    cam = camera_for(rows, cols)
    rng = np.random.default_rng(9)
    cur, _, sources, mots = _case("37x53", "yaw", 3)
    cur, sources = cur.copy(), [s.copy() for s in sources]
    for a in [cur] + sources:
        pick = rng.random((rows, cols)) < 0.1
        a[pick] = rng.choice(FC.SPECIALS, int(pick.sum()))
    cur.ravel()[:FC.SPECIALS.size] = FC.SPECIALS
    for radius in (0, 2):
        want = FC.check_consistency(torch, engine, cur, sources, cam, mots, MAX_DIFF, radius, 1, 1)
        assert 0 < want["counts"][1] < want["counts"][0] and np.isnan(want["out"]).any()
    d = rng.uniform(8.0, 12.0, (rows, cols)).astype(np.float32)
    eight, ident = _eight_sources(d)
    for mc, mx in ((0, 8), (0, 0), (8, 8), (2, 2), (2, 1)):
        want = FC.check_consistency(torch, engine, d, eight, cam, ident, 1.0, 0, mc, mx)
        assert (want["classes"] == 0xE4E4).all() and want["counts"][1] == (d.size if mc <= 2 and mx >= 2 else 0)
    FC.check_consistency(torch, engine, cur, [cur, sources[0]], cam, [FC.IDENTITY, mots[0]], 0.0, 1, 1, 0, self_source=(0,))


@gpu
def test_invalid_arguments_are_named_and_nothing_is_enqueued(pm, engine):
    """PM_ERR_INVALID_ARG with pm_last_error naming the argument; every output keeps its guard pattern."""
    import torch
    rows, cols = 16, 24
    lib, h = engine.lib, engine.h
    disp = torch.full((rows, cols), 10.0, dtype=torch.float32, device="cuda")
    other = torch.full((2, rows, cols), 10.0, dtype=torch.float32, device="cuda")
    outs = {k: FC.Guarded(torch, n) for k, n in (("out", 4 * rows * cols), ("cls", 2 * rows * cols), ("res", 4 * rows * cols), ("c", 8))}
    good = camera_for(rows, cols)
    host = (C.c_int * 2)(-5, -5)
    UNSET = object()
    two = [other[0].data_ptr(), other[1].data_ptr()]

    def call(cam=good, opt=(1.0, 1, 1, 0), d=UNSET, src=two, n=None, mot=UNSET, shape=(rows, cols), out=UNSET, cls=UNSET,
             res=UNSET, c=UNSET, hc=host):
        cc = pm.cloud_camera(cam)
        o = pm.PmConsistencyOptions(*opt) if opt is not None else None
        pick = lambda v, default: default if v is UNSET else v
        arr = (C.c_void_p * len(src))(*src) if src is not None else None
        count = len(src) if n is None else n
        mots = pick(mot, [FC.IDENTITY] * (len(src) if src is not None else 1))
        m = (pm.PmMotion * len(mots))(*[pm.as_motion(v) for v in mots]) if mots is not None else None
        return lib.pm_filter_consistency(h, C.byref(cc) if cc is not None else None, C.byref(o) if o is not None else None,
                                         pick(d, disp.data_ptr()), count, arr, m, shape[0], shape[1], pick(out, outs["out"].ptr),
                                         pick(cls, outs["cls"].ptr), pick(res, outs["res"].ptr), pick(c, outs["c"].ptr), hc)

    def refused(rc, word, status=pm.PM_ERR_INVALID_ARG):
        text = lib.pm_last_error(h).decode()
        assert rc == status and word in text, (rc, word, text)

    refused(call(cam=None), "camera")
    refused(call(opt=None), "options")
    refused(call(d=None), "d_disp")
    refused(call(src=None, n=2, mot=[FC.IDENTITY] * 2), "d_sources")
    refused(call(mot=None), "motions")
    refused(call(src=[two[0], None]), "d_sources[1]")
    for i, name in enumerate(("fx", "fy", "cx", "cy", "baseline")):
        for bad in (np.nan, np.inf, -np.inf):
            cam = list(good)
            cam[i] = bad
            refused(call(cam=cam), name)
    refused(call(cam=(0.0,) + good[1:]), "fx")
    refused(call(cam=(good[0], 0.0) + good[2:]), "fy")
    refused(call(src=[], n=0, mot=[FC.IDENTITY]), "n_sources")
    refused(call(src=two * 4 + two[:1], mot=[FC.IDENTITY] * 9), "n_sources")
    refused(call(n=-1), "n_sources")
    for i in range(12):
        for bad in (np.nan, np.inf, -np.inf):
            R, t = np.eye(3).ravel(), np.zeros(3)
            (R if i < 9 else t)[i if i < 9 else i - 9] = bad
            refused(call(mot=[FC.IDENTITY, (R, t)]), ("R[%d]" % i if i < 9 else "t[%d]" % (i - 9)) + " of motions[1]")
    for bad in (np.nan, np.inf, -0.5):
        refused(call(opt=(bad, 1, 1, 0)), "max_diff")
    refused(call(opt=(1.0, -1, 1, 0)), "radius")
    refused(call(opt=(1.0, 3, 1, 0)), "radius")
    refused(call(opt=(1.0, 1, -1, 0)), "min_consistent")
    refused(call(opt=(1.0, 1, 3, 0)), "min_consistent")
    refused(call(opt=(1.0, 1, 1, -1)), "max_conflicts")
    refused(call(opt=(1.0, 1, 1, 9)), "max_conflicts")
    refused(call(shape=(0, cols)), "empty")
    refused(call(shape=(rows, 0)), "empty")
    refused(call(shape=(rows, -3)), "empty")
    refused(call(out=None, cls=None, res=None, c=None, hc=None), "no output")
    refused(call(out=two[1]), "d_sources[1]")
    refused(call(src=[two[0], disp.data_ptr()], out=disp.data_ptr()), "d_sources[1]")  # in place on a map that is a source
    refused(call(shape=(70000, 40000)), "exceed", pm.PM_ERR_SIZE)
    engine.synchronize()
    for buf in outs.values():
        buf.read(np.uint8, 0)
    assert tuple(host) == (-5, -5) and (disp.cpu().numpy() == 10.0).all() and (other.cpu().numpy() == 10.0).all()
    # and the same arguments made good do run
    assert call() == pm.PM_OK and tuple(host) == (rows * cols, rows * cols)
    assert call(src=[two[0], disp.data_ptr()]) == pm.PM_OK  # a source may be the current map


@gpu
def test_consistency_scratch_is_owned_by_the_handle(pm):
    """The 16 bytes of the two counts are ONE handle-owned allocation through csrc/pm_devbuf.hpp: made on first use, reused
    whatever the size of the maps, gone with the handle."""
    import torch
    lib = pm.load()
    live = lambda: (lib.pm_debug_live_device_allocations(), lib.pm_debug_live_device_bytes())
    before = live()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        base = live()
        small = torch.full((37, 53), 3.0, dtype=torch.float32, device="cuda")
        large = torch.full((300, 500), 3.0, dtype=torch.float32, device="cuda")
        cls = torch.zeros((300, 500), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        run = lambda t, n: e.filter_consistency(camera_for(*t.shape), t.data_ptr(), [t.data_ptr()] * n, [FC.IDENTITY] * n,
                                                t.shape[0], t.shape[1], d_classes=cls.data_ptr(), want_counts=True)
        assert run(small, 1) == (37 * 53, 37 * 53)
        first = live()
        assert first == (base[0] + 1, base[1] + 16)
        assert run(large, 8) == (300 * 500, 300 * 500) and live() == first
        assert run(small, 3) == (37 * 53, 37 * 53) and live() == first
        assert (cls[:37 * 53 // 500].cpu().numpy() == 0b010101).all()
    assert live() == before


# ---- 4. through a sequence: three matches of one pair, the first judged by the other two -------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["scalar", "planes"])
def test_a_map_is_filtered_against_two_other_matches_on_the_handles_stream(pm, synth, mode):
    """Three handles that differ in noise_seed match one pair; map 1 is filtered against maps 2 and 3 with the identity motion
    on the first handle's stream, nothing copied: the result equals the definition on the downloaded maps."""
    import torch
    rows, cols = 96, 128
    p = synth.make_pair(3, rows=rows, cols=cols, n_points=40, dilate_factor=2)
    cam = camera_for(rows, cols)
    kw = dict(mode=pm.PM_MODE_PLANES) if mode == "planes" else {}
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    L, R, SL, SR = up(p["left"]), up(p["right"]), up(p["seed_l"]), up(p["seed_r"])
    D = torch.zeros((3, 2, rows, cols), dtype=torch.float32, device="cuda")
    out = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    cls = torch.zeros((rows, cols), dtype=torch.int16, device="cuda")
    res = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    engines = [pm.Engine(pm.default_params(0, patch=5, patchmatch_iters=2, max_disp=32, noise_seed=123 + 1000 * k, **kw),
                         max_rows=rows, max_cols=cols) for k in range(3)]
    try:
        for k, e in enumerate(engines):
            e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), D[k, 0].data_ptr(),
                           D[k, 1].data_ptr())
        for e in engines[1:]:
            e.synchronize()  # the first handle's stream is not ordered behind the other two
        e = engines[0]
        n = e.filter_consistency(cam, D[0, 0].data_ptr(), [D[1, 0].data_ptr(), D[2, 0].data_ptr()], [FC.IDENTITY] * 2, rows, cols,
                                 max_diff=1.0, radius=1, min_consistent=2, max_conflicts=0, d_out=out.data_ptr(),
                                 d_classes=cls.data_ptr(), d_residual=res.data_ptr(), want_counts=True)
        e.synchronize()
    finally:
        for e in engines:
            e.close()
    maps = D.cpu().numpy()
    assert not np.array_equal(maps[0, 0], maps[1, 0]) and not np.array_equal(maps[1, 0], maps[2, 0])  # the seeds do differ
    want = CR.filter_consistency(maps[0, 0], [maps[1, 0], maps[2, 0]], cam, [FC.IDENTITY] * 2, 1.0, 1, 2, 0)
    assert want["counts"][0] > 0.25 * rows * cols and 0 < want["counts"][1] < want["counts"][0]
    assert n == tuple(int(v) for v in want["counts"])
    assert np.array_equal(FC.bits(out.cpu().numpy()), FC.bits(want["out"]))
    assert np.array_equal(cls.cpu().numpy().view(np.uint16), want["classes"])
    assert np.array_equal(FC.bits(res.cpu().numpy()), FC.bits(want["residual"]))


@gpu
def test_fuzz_consistency_one_short_seeded_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_consistency.py"), "--cases", "20", "--seed", "4"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
