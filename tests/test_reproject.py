"""Temporal seeds: the left map of one frame carried into the next frame's two seed maps (include/pm/imaging.h:
pm_reproject_disparity).

CPU tests pin the definition (tests/reproject_ref.py) against analytic cases and run the kernels' own per-thread code
(csrc/pm_reproject_body.hpp) on the host under ASan / UBSan, blocks forwards and backwards.  GPU tests hold the kernels to
the definition with tolerance 0 -- every operation of the definition is one IEEE rounding, the build uses
-ffp-contract=off, and only integer maximum and integer addition cross workgroups -- with guard bands around every output.
Every case is first shown to be non-trivial ON THE DEFINITION ALONE: enough pixels > 0, a collision where surfaces are
meant to collide, a closed hole where the close is meant to act."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import reproject_ref as RR
from conftest import ROOT
from cpp_build import build_host_kernel
from host_run import assert_program_compares, dump_case, flat_motions
from pointcloud_ref import camera_for

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_reproject as FR  # noqa: E402  (check_reproject: the device-against-definition comparison)

gpu = pytest.mark.gpu

CAM = (412.7, 398.3, 39.7, 24.4, 0.12)  # the camera of the analytic cases, for a 48x80 map
FXB = np.float64(CAM[0]) * np.float64(CAM[4])


def two_level(rows, cols, seed=0, far=6.0, near=14.0, zeros=0.08, very_near=False):
    """A far background with a near box in the middle, both with a little relief, and some pixels without a value."""
    rng = np.random.default_rng(seed)
    d = np.full((rows, cols), far, np.float32)
    d[rows // 4:rows - rows // 4, cols // 3:cols - cols // 3] = near
    d += rng.uniform(-0.2, 0.2, (rows, cols)).astype(np.float32)
    if very_near:  # a surface a quarter of a metre away: a small advance puts it behind the camera
        d[:rows // 3, :cols // 4] = 200.0
    d[rng.random((rows, cols)) < zeros] = 0.0
    return d


def motions(camera, depth):
    I = np.eye(3)
    return {
        "identity": FR.IDENTITY,
        "baseline": (I.ravel(), np.array([-camera[4], 0.0, 0.0])),
        "advance": (I.ravel(), np.array([0.0, 0.0, -0.1 * depth])),
        "yaw": (FR.rotation((0, 1, 0), 2.0).ravel(), np.zeros(3)),
        "roll": (FR.rotation((0, 0, 1), 7.0).ravel(), np.zeros(3)),
        "behind": (I.ravel(), np.array([0.0, 0.0, -0.3])),
        "gone": (I.ravel(), np.array([100.0, 0.0, 0.0])),
    }


# ---- 1. the definition ------------------------------------------------------------------------------------------------
def test_definition_identity_returns_the_map_bit_for_bit():
    """20 random 48x80 maps, 20 % zeros, d in 0.01 .. 128: R = I, t = 0 lands every pixel on itself with its own value."""
    rng = np.random.default_rng(11)
    for _ in range(20):
        d = rng.uniform(0.01, 128.0, (48, 80)).astype(np.float32)
        d[rng.random((48, 80)) < 0.2] = 0.0
        for r in (0, 1):
            out = RR.reproject(d, CAM, *FR.IDENTITY, close_radius=r)
            assert np.array_equal(FR.bits(out["splat_l"]), FR.bits(d))
            assert (out["hits_l"] == (d > 0)).all()
        out = RR.reproject(d, CAM, *FR.IDENTITY, close_radius=0)
        assert np.array_equal(FR.bits(out["seed_l"]), FR.bits(d)) and out["counts"][0] == (d > 0).sum()


def test_definition_baseline_shift_and_advance():
    d = np.full((48, 80), 20.0, np.float32)
    # the new left camera where the old right camera was: a constant-20 map moves by 20 columns
    out = RR.reproject(d, CAM, np.eye(3), (-0.12, 0.0, 0.0), close_radius=0)
    assert (out["seed_l"][:, :60] == 20.0).all() and (out["seed_l"][:, 60:] == 0).all() and out["counts"][0] == 48 * 60
    # an advance by 10 % of the range: the disparity grows to 20 / 0.9 and the image spreads about the principal point
    Z = FXB / 20.0
    t = (0.0, 0.0, -0.1 * Z)
    want = np.float32(20.0 / 0.9)
    raw = RR.reproject(d, CAM, np.eye(3), t, close_radius=0)
    hit = raw["seed_l"] > 0
    assert (~hit).sum() == 672 and np.abs(raw["seed_l"][hit] - want).max() <= 4e-6
    out = RR.reproject(d, CAM, np.eye(3), t, close_radius=1)
    assert (out["seed_l"] > 0).all() and np.abs(out["seed_l"] - want).max() <= 4e-6 and out["counts"][0] == 48 * 80
    assert np.array_equal(out["seed_l"][hit], raw["seed_l"][hit])  # the close never alters a pixel that was hit
    # the right view: x - 22.22 rounds to x - 22, so columns 0 .. 57 are landed on; its own close then reaches column 58
    assert (out["splat_r"][:, :58] > 0).all() and (out["splat_r"][:, 58:] == 0).all()
    assert (out["seed_r"][:, :59] > 0).all() and (out["seed_r"][:, 59:] == 0).all() and out["counts"][1] == 48 * 59


def test_definition_the_near_surface_wins_a_collision():
    """A step edge moved sideways: near (30) moves 30 columns, far (10) moves 10, so near lands on far's pixels."""
    d = np.full((48, 80), 10.0, np.float32)
    d[:, 50:] = 30.0
    out = RR.reproject(d, CAM, np.eye(3), (-0.12, 0.0, 0.0), close_radius=0)
    both = out["hits_l"] > 1
    assert both.sum() == 48 * 20 and (out["seed_l"][both] == 30.0).all()  # columns 20 .. 39: far from 30 .. 49, near from 50 .. 69
    assert (out["seed_l"][:, :20] == 10.0).all() and (out["seed_l"][:, 40:50] == 30.0).all() and (out["seed_l"][:, 50:] == 0).all()


def test_definition_close_and_special_values():
    S = np.zeros((9, 11), np.float32)
    S[4, 5], S[0, 0], S[8, 10] = 7.0, 3.0, 5.0
    for r in range(4):
        C_ = RR.close(S, r)
        want = np.zeros_like(S)
        want[max(4 - r, 0):5 + r, max(5 - r, 0):6 + r] = 7.0
        want[:r + 1, :r + 1] = np.maximum(want[:r + 1, :r + 1], 3.0)
        want[8 - r:, 10 - r:] = np.maximum(want[8 - r:, 10 - r:], 5.0)
        assert np.array_equal(C_, want), r
    d = np.full((16, 24), 9.0, np.float32)
    d.ravel()[:FR.SPECIALS.size] = FR.SPECIALS
    d[3, :] = 2.0  # below min_disp
    out = RR.reproject(d, camera_for(16, 24), *FR.IDENTITY, min_disp=5.0, close_radius=0)
    assert np.array_equal(out["seed_l"] > 0, (d >= 5.0) & np.isfinite(d)) and np.isinf(d).sum() == 1
    assert out["seed_l"].ravel()[5] == 0  # +inf: a point at range 0 has no finite disparity
    cut = RR.reproject(d, camera_for(16, 24), *FR.IDENTITY, max_disp=5.0, close_radius=0)
    assert np.array_equal(cut["seed_l"] > 0, (d > 0) & (d <= 5.0))


def test_relative_motion_of_the_definition():
    A, B = np.eye(4), np.eye(4)
    A[:3, :3], A[:3, 3] = FR.rotation((0, 1, 0), 10), (1.0, 2.0, 3.0)
    B[:3, :3], B[:3, 3] = FR.rotation((1, 1, 0), -25), (-0.5, 0.2, 4.0)
    R, t = RR.relative_motion(A, B)
    T = np.linalg.inv(B) @ A
    assert np.abs(R.reshape(3, 3) - T[:3, :3]).max() < 1e-14 and np.abs(t - T[:3, 3]).max() < 1e-14


# ---- 2. the kernels' own per-thread code, run on the host ----------------------------------------------------------------
@pytest.fixture(scope="module")
def host_reproject_exe(tmp_path_factory):
    """tests/cpp/reproject_host_main.cpp: csrc/pm_reproject_body.hpp compiled for the host alone, with the sanitizers."""
    return build_host_kernel(tmp_path_factory.mktemp("reprojecthost") / "reproject_host_main", "reproject_host_main.cpp")


def _dump_case(path, disp, cam, motion, min_disp, max_disp, r, shift):
    want = RR.reproject(disp, cam, motion[0], motion[1], min_disp, max_disp, r)
    dump_case(path, [*disp.shape, *cam, *flat_motions([motion], 1), min_disp, max_disp, r, shift],
              disp=disp, want_seed_l=want["seed_l"], want_seed_r=want["seed_r"], want_counts=want["counts"])
    return want


def test_kernel_code_on_the_host_equals_the_definition(host_reproject_exe, tmp_path):
    """Every thread of the four launches over whole maps on the CPU, forwards and backwards: both seed maps and both counts
    equal the .npy dumps of the definition byte for byte, and AddressSanitizer / UBSan see every access into buffers (the
    tile included) of exactly the size the stage may touch."""
    tw, th = 64, 16
    cases = []  # rows, cols, motion, map kwargs, min_disp, max_disp, r, shift
    for k, (shape, name, r, shift) in enumerate([((1, 1), "identity", 1, 0), ((1, 7), "identity", 3, 1), ((37, 53), "yaw", 1, 0),
                                                 ((37, 53), "baseline", 2, 3), ((37, 53), "roll", 0, 2), ((64, 96), "advance", 1, 0),
                                                 ((th + 1, 2 * tw + 3), "behind", 3, 1), ((37, 53), "gone", 1, 0),
                                                 ((9, 300), "yaw", 2, 0)]):
        rows, cols = shape
        cam = camera_for(rows, cols)
        disp = two_level(rows, cols, seed=k, very_near=name == "behind")
        disp.ravel()[:min(FR.SPECIALS.size, disp.size - 1)] = FR.SPECIALS[:min(FR.SPECIALS.size, disp.size - 1)]
        cases.append((disp, cam, motions(cam, FXB / 6.0)[name], 5.0 if k == 3 else 0.0, 15.0 if k == 5 else 0.0, r, shift))
    seeds = 0
    for k, c in enumerate(cases):
        d = str(tmp_path / ("case%d" % k))
        seeds += int(_dump_case(d, *c)["counts"].sum())
        r = subprocess.run([host_reproject_exe, d], capture_output=True, text=True)
        assert r.returncode == 0, (k, r.stderr[-3000:])
    assert seeds > 10000
    # the program does compare: one flipped bit in an expectation is a mismatch, not a pass
    assert_program_compares(host_reproject_exe, str(tmp_path / "case2"), [("want_seed_r", np.uint32, "seed_r differs")])


def test_headers_declare_and_the_library_exports_the_reproject_functions(pm):
    text = open(os.path.join(ROOT, "include", "pm", "imaging.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = pm.load()
    assert re.search(r"\bint\s+pm_reproject_disparity\s*\(\s*pm_handle\s*\*", text)
    assert "typedef struct pm_motion" in text and "typedef struct pm_reproject_options" in text
    testing = open(os.path.join(ROOT, "include", "pm", "testing.h")).read()
    assert re.search(r"\bvoid\s+pm_debug_reproject_constants\s*\(\s*int\s*\*", testing)
    for name in ("pm_reproject_disparity", "pm_debug_reproject_constants"):
        assert name in pm.EXPORTS and hasattr(lib, name), name
    assert C.sizeof(pm.PmMotion) == 96 and C.sizeof(pm.PmReprojectOptions) == 12
    tw, th = pm.reproject_constants()
    assert tw >= 8 and th >= 8


# ---- 3. device parity ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        yield e


def _nontrivial(want, empty=False, collide=False, closes=False):
    """The conditions of a case, on the definition's output alone."""
    share = float((want["seed_l"] > 0).mean())
    if empty:
        assert share == 0 and not want["seed_r"].any() and (want["counts"] == 0).all()
        return
    assert share >= 0.25, share
    if collide:
        assert (want["hits_l"] > 1).any()
    if closes:
        assert ((want["splat_l"] == 0) & (want["seed_l"] > 0)).any()


def _shape_of(pm, name):
    tw, th = pm.reproject_constants()
    return {"1x1": (1, 1), "1x7": (1, 7), "37x53": (37, 53), "64x96": (64, 96), "tile": (th + 1, 2 * tw + 3), "9x300": (9, 300)}[name]


SMALL = [(s, m) for s in ("1x1", "1x7") for m in ("identity", "advance")]
FULL = [(s, m) for s in ("37x53", "64x96", "tile") for m in ("identity", "baseline", "advance", "yaw", "roll", "behind", "gone")]


@gpu
@pytest.mark.parametrize("shape,motion", SMALL + FULL + [("1x7", "gone"), ("9x300", "yaw"), ("9x300", "baseline")],
                         ids=lambda v: v)
def test_reproject_equals_the_definition(pm, engine, shape, motion):
    """Five shapes (one pixel, one short row, no multiple of a tile or of 4, whole tiles, one row and three columns beyond
    tiles) x seven motions, and a row longer than the 256 pixels one wavefront of the splat takes; close_radius 1 and 2;
    maps, d_counts and host counts all at tolerance 0."""
    import torch
    rows, cols = _shape_of(pm, shape)
    cam = camera_for(rows, cols)
    small = rows * cols < 16
    if small:  # a surface so far that an advance moves no pixel of a short row out of it
        disp = np.full((rows, cols), 1.5, np.float32)
    else:
        disp = two_level(rows, cols, seed=rows + cols, very_near=motion == "behind")
    mot = motions(cam, FXB / (1.5 if small else 6.0))[motion]
    for r in (1, 2):
        want = RR.reproject(disp, cam, mot[0], mot[1], close_radius=r)
        _nontrivial(want, empty=motion == "gone", collide=motion == "baseline" and not small,
                    closes=not small and motion in ("advance", "yaw", "roll", "behind"))
        FR.check_reproject(torch, engine, disp, cam, mot, close_radius=r, want=want)
    if motion == "behind":
        gone = RR.splat_left(np.where(disp == 200.0, disp, 0).astype(np.float32), cam, *mot)[0]
        assert (disp == 200.0).sum() > 20 and not gone.any()  # the near surface did pass behind the camera


@gpu
@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_close_radius_with_holes_on_tile_borders_and_corners(pm, engine, r):
    """Identity motion over two and a bit tiles each way: isolated one-pixel holes on either side of a tile's border, around
    its corner and in the image's corners, and a 7x7 hole across a tile corner of which radius r closes the outer r rings (its
    centre stays open at every radius).  The values differ from pixel to pixel, so a tap from the wrong place shows."""
    import torch
    tw, th = pm.reproject_constants()
    rows, cols = 2 * th + 3, 2 * tw + 5
    rng = np.random.default_rng(5)
    disp = rng.uniform(5.0, 9.0, (rows, cols)).astype(np.float32)
    holes = [(th - 1, 5), (th, 9), (7, tw - 1), (3, tw), (th - 1, tw - 1), (th, tw + 2), (th + 2, tw), (0, 0), (0, cols - 1),
             (rows - 1, 0), (rows - 1, cols - 1), (2 * th - 1, 2 * tw), (2 * th, 2 * tw - 1)]
    for y, x in holes:
        disp[y, x] = 0.0
    disp[th - 3:th + 4, 2 * tw - 3:2 * tw + 4] = 0.0
    cam = camera_for(rows, cols)
    want = RR.reproject(disp, cam, *FR.IDENTITY, close_radius=r)
    assert np.array_equal(want["splat_l"], disp)
    closed = (disp == 0) & (want["seed_l"] > 0)
    if r == 0:
        assert not closed.any()
    else:
        assert all(closed[y, x] for y, x in holes)
        ring = 49 - (7 - 2 * r) ** 2 if r < 4 else 49
        assert closed.sum() == len(holes) + ring
    assert (want["seed_l"] > 0).mean() >= 0.25
    FR.check_reproject(torch, engine, disp, cam, FR.IDENTITY, close_radius=r, want=want)


@gpu
def test_special_values_options_and_each_output_alone(pm, engine):
    """Sources 0, -0.0, negative, NaN, +inf, subnormal and below min_disp; max_disp cutting the near surface after an
    advance; an unaligned source; then every output asked for alone."""
    import torch
    rows, cols = 37, 53
    cam = camera_for(rows, cols)
    rng = np.random.default_rng(9)
    disp = two_level(rows, cols, seed=3)
    pick = rng.random((rows, cols)) < 0.1
    disp[pick] = rng.choice(FR.SPECIALS, int(pick.sum()))
    disp.ravel()[:FR.SPECIALS.size] = FR.SPECIALS
    disp[5, :] = 2.0
    adv = motions(cam, FXB / 6.0)["advance"]
    want = RR.reproject(disp, cam, *adv, min_disp=5.0, close_radius=1)
    free = RR.reproject(disp, cam, *adv, close_radius=1)
    assert 0.25 <= (want["seed_l"] > 0).mean() and want["counts"][0] < free["counts"][0]  # min_disp drops row 5
    for off in (0, 1):
        FR.check_reproject(torch, engine, disp, cam, adv, min_disp=5.0, close_radius=1, offset_floats=off, want=want)
    cut = RR.reproject(disp, cam, *adv, max_disp=10.0, close_radius=1)
    assert 0.25 <= (cut["seed_l"] > 0).mean() and cut["seed_l"].max() <= 10.0 < free["seed_l"].max()
    FR.check_reproject(torch, engine, disp, cam, adv, max_disp=10.0, close_radius=1, want=cut)
    for only in ("seed_l", "seed_r", "d_counts", "counts"):
        FR.check_reproject(torch, engine, disp, cam, adv, close_radius=1, outputs=(only,), want=free)


@gpu
def test_invalid_arguments_are_named_and_nothing_is_enqueued(pm, engine):
    """PM_ERR_INVALID_ARG with pm_last_error naming the argument; every output keeps its guard pattern."""
    import torch
    rows, cols = 16, 24
    lib, h = engine.lib, engine.h
    disp = torch.full((rows, cols), 10.0, dtype=torch.float32, device="cuda")
    outs = {k: FR.Guarded(torch, n) for k, n in (("l", 4 * rows * cols), ("r", 4 * rows * cols), ("c", 8))}
    good = camera_for(rows, cols)
    host = (C.c_int * 2)(-5, -5)
    UNSET = object()

    def call(cam=good, mot=FR.IDENTITY, opt=(0.0, 0.0, 1), d=UNSET, shape=(rows, cols), l=UNSET, r=UNSET, c=UNSET, hc=host):
        cc, m = pm.cloud_camera(cam), pm.as_motion(mot)
        o = pm.PmReprojectOptions(*opt) if opt is not None else None
        pick = lambda v, default: default if v is UNSET else v
        return lib.pm_reproject_disparity(h, C.byref(cc) if cc is not None else None, C.byref(m) if m is not None else None,
                                          C.byref(o) if o is not None else None, pick(d, disp.data_ptr()), shape[0], shape[1],
                                          pick(l, outs["l"].ptr), pick(r, outs["r"].ptr), pick(c, outs["c"].ptr), hc)

    def refused(rc, word, status=pm.PM_ERR_INVALID_ARG):
        text = lib.pm_last_error(h).decode()
        assert rc == status and word in text, (rc, word, text)

    refused(call(cam=None), "camera")
    refused(call(mot=None), "motion")
    refused(call(opt=None), "options")
    refused(call(d=None), "d_disp")
    for i, name in enumerate(("fx", "fy", "cx", "cy", "baseline")):
        for bad in (np.nan, np.inf, -np.inf):
            cam = list(good)
            cam[i] = bad
            refused(call(cam=cam), name)
    refused(call(cam=(0.0,) + good[1:]), "fx")
    refused(call(cam=(good[0], 0.0) + good[2:]), "fy")
    for i in range(12):
        for bad in (np.nan, np.inf, -np.inf):
            R, t = np.eye(3).ravel(), np.zeros(3)
            (R if i < 9 else t)[i if i < 9 else i - 9] = bad
            refused(call(mot=(R, t)), "R[%d]" % i if i < 9 else "t[%d]" % (i - 9))
    refused(call(opt=(np.nan, 0.0, 1)), "min_disp")
    refused(call(opt=(-1.0, 0.0, 1)), "min_disp")
    refused(call(opt=(0.0, np.nan, 1)), "max_disp")
    refused(call(opt=(0.0, -0.5, 1)), "max_disp")
    refused(call(opt=(0.0, 0.0, -1)), "close_radius")
    refused(call(opt=(0.0, 0.0, 4)), "close_radius")
    refused(call(shape=(0, cols)), "empty")
    refused(call(shape=(rows, 0)), "empty")
    refused(call(shape=(rows, -3)), "empty")
    refused(call(l=None, r=None, c=None, hc=None), "no output")
    refused(call(l=disp.data_ptr()), "d_seed_l")
    refused(call(r=disp.data_ptr()), "d_seed_r")
    refused(call(shape=(70000, 40000), l=None, r=None), "exceed", pm.PM_ERR_SIZE)
    engine.synchronize()
    for buf in outs.values():
        buf.read(np.uint8, 0)
    assert tuple(host) == (-5, -5) and (disp.cpu().numpy() == 10.0).all()
    # and the same arguments made good do run
    assert call() == pm.PM_OK and tuple(host) == (rows * cols, rows * (cols - 10 + 1))  # the close reaches one column further


@gpu
def test_reproject_scratch_is_owned_by_the_handle(pm):
    """The two splat maps and the counts are ONE handle-owned allocation through csrc/pm_devbuf.hpp: made on first use,
    reused at the same size (a second call allocates nothing), grown for a larger map or for the third map of a call without
    d_seed_l, gone with the handle."""
    import torch
    lib = pm.load()
    live = lambda: (lib.pm_debug_live_device_allocations(), lib.pm_debug_live_device_bytes())
    before = live()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        base = live()
        small = torch.full((37, 53), 3.0, dtype=torch.float32, device="cuda")
        large = torch.full((300, 500), 3.0, dtype=torch.float32, device="cuda")
        out = torch.zeros((2, 300, 500), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        run = lambda t, **kw: e.reproject_disparity(camera_for(*t.shape), FR.IDENTITY, t.data_ptr(), t.shape[0], t.shape[1],
                                                    want_counts=True, **kw)
        # a constant 3: the right view is landed on in all but the last 3 columns, and the close reaches r of those
        assert run(small, d_seed_l=out[0].data_ptr(), d_seed_r=out[1].data_ptr()) == (37 * 53, 37 * 51)
        first = live()
        assert first[0] == base[0] + 1 and first[1] >= base[1] + 8 * 37 * 53
        assert run(small, d_seed_l=out[0].data_ptr(), d_seed_r=out[1].data_ptr(), close_radius=3) == (37 * 53, 37 * 53)
        assert live() == first
        assert run(small, d_seed_r=out[1].data_ptr()) == (37 * 53, 37 * 51)  # the closed left seed in scratch: a third map
        third = live()
        assert third[0] == first[0] and third[1] > first[1]
        assert run(large, d_seed_l=out[0].data_ptr()) == (300 * 500, 300 * 498)
        grown = live()
        assert grown[0] == first[0] and grown[1] > third[1]
        assert run(small) == (37 * 53, 37 * 51)
        assert live() == grown
    assert live() == before


# ---- 4. through a sequence: the handle's stream, an event, pm_submit_device_after ----------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["scalar", "planes"])
def test_reprojected_seeds_reach_the_next_frame_through_an_event(pm, synth, mode):
    """Match frame A, reproject its left map on the handle's stream, record an event there, submit frame B behind that event
    with the device seeds: both maps of B equal, bit for bit, a match_device of B seeded with the numpy definition's maps
    uploaded from the host."""
    import torch
    rows, cols = 64, 96
    a, b = (synth.make_pair(k, rows=rows, cols=cols, n_points=40, dilate_factor=2) for k in (3, 4))
    cam = camera_for(rows, cols)
    mot = (FR.rotation((0, 1, 0), 0.4).ravel(), np.array([0.01, 0.0, -0.05]))
    kw = dict(mode=pm.PM_MODE_PLANES) if mode == "planes" else {}
    prm = pm.default_params(0, patch=5, patchmatch_iters=2, max_disp=32, **kw)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    AL, AR, BL, BR = up(a["left"]), up(a["right"]), up(b["left"]), up(b["right"])
    ASL, ASR = up(a["seed_l"]), up(a["seed_r"])  # frame A starts from the pair's own sparse seeds
    D = torch.zeros((6, rows, cols), dtype=torch.float32, device="cuda")  # A's maps, the seeds, B's maps
    torch.cuda.synchronize()
    with pm.Engine(prm, max_rows=rows, max_cols=cols, max_batch=2) as e:
        e.match_device(1, AL.data_ptr(), AR.data_ptr(), rows, cols, ASL.data_ptr(), ASR.data_ptr(), D[0].data_ptr(), D[1].data_ptr())
        e.reproject_disparity(cam, mot, D[0].data_ptr(), rows, cols, min_disp=0.5, close_radius=1, d_seed_l=D[2].data_ptr(),
                              d_seed_r=D[3].data_ptr())
        ready = torch.cuda.Event()
        ready.record(torch.cuda.ExternalStream(e.stream()))
        e.submit_device(BL.data_ptr(), BR.data_ptr(), rows, cols, D[2].data_ptr(), D[3].data_ptr(), D[4].data_ptr(),
                        D[5].data_ptr(), tag=7, ready_event=ready.cuda_event)
        while e.in_flight():
            e.collect_device()
        e.synchronize()
        got = D.cpu().numpy()
        want = RR.reproject(got[0], cam, mot[0], mot[1], min_disp=0.5, close_radius=1)
        assert (want["seed_l"] > 0).mean() >= 0.25 and (want["seed_r"] > 0).mean() >= 0.25
        assert np.array_equal(FR.bits(got[2]), FR.bits(want["seed_l"])) and np.array_equal(FR.bits(got[3]), FR.bits(want["seed_r"]))
        SL, SR = up(want["seed_l"]), up(want["seed_r"])
        E = torch.zeros((2, rows, cols), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        e.match_device(1, BL.data_ptr(), BR.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), E[0].data_ptr(), E[1].data_ptr())
        e.synchronize()
        ref = E.cpu().numpy()
    assert np.array_equal(FR.bits(got[4]), FR.bits(ref[0])) and np.array_equal(FR.bits(got[5]), FR.bits(ref[1]))
    assert (ref[0] > 0).mean() > 0.25


@gpu
def test_fuzz_reproject_one_short_seeded_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_reproject.py"), "--cases", "20", "--seed", "4"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
