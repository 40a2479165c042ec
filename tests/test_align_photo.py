"""pm_bgr_luma, pm_align_photo_evaluate, pm_align_sums_blend and pm_align_color_disparity (include/pm/imaging.h, DESIGN.md section
8c-14): the photometric term of the dense alignment and the loop that blends it into pm_align_disparity's.  The definition is
tests/align_photo_ref.py; everything is held to it with tolerance 0.

1. the definition alone, on analytic scenes (a textured plane at 2 m, and tests/test_align.py's pyramid scene): lumas, constant
   images, every class, the blend, a frame against itself, the degenerate plane that the geometric term cannot solve, chains.
2. the kernels' per-thread code compiled for the HOST with the sanitizers (tests/cpp/align_photo_host_main.cpp).
3. the device against the definition (marked gpu), guard bands round every buffer.

`python tests/test_align_photo.py` writes profiles/align_color_accuracy.txt from the definition."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import align_photo_ref as AP
import align_ref as AR
import tsdf_color_ref as TC
import tsdf_ref as TR
import test_align as TA
from conftest import ROOT
from cpp_build import build_host_kernel
from host_run import assert_program_compares, dump_case
from test_align import CAM, COLS, GRID, IDENT, I3, RAY, ROWS, Z0, motion_error, perturbed, rotation
from test_reproject import motions

FA = TA.FA
gpu = pytest.mark.gpu
PROFILE = os.path.join(ROOT, "profiles", "align_color_accuracy.txt")
LAMBDA, HUBER_LEVELS = 0.03, 20.0
OPT = AP.color_options(**dict(TA.OPT, huber_levels=HUBER_LEVELS, lam=LAMBDA))
GEO_OPT = TA.OPT
PHOTO_OPT = AP.photo_options(max_diff=TA.OPT["max_diff"], huber_levels=HUBER_LEVELS)
bits = lambda a: np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype == np.float32 else np.uint64)


# ---- the scenes -----------------------------------------------------------------------------------------------------------------
def render_plane(pose, rows=ROWS, cols=COLS, cam=CAM):
    """The plane at world Z = Z0 alone, seen from `pose` (X_cam = R X_world + t), by exact intersection in binary64 until the final
    rounding; +0.0 where the ray does not meet it in front of the camera."""
    fx, fy, cx, cy, baseline = (np.float64(v) for v in cam)
    R = np.asarray(pose[0], np.float64).reshape(3, 3)
    c = -(R.T @ np.asarray(pose[1], np.float64))
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    wd = np.stack(np.broadcast_arrays((x - cx) / fx, (y - cy) / fy, np.ones((rows, cols))), -1) @ R
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (Z0 - c[2]) / wd[..., 2]
        return np.where(s > 0, (fx * baseline) / s, 0.0).astype(np.float32)


def texture(X, Y, Z):
    """The analytic texture of world position, in levels -> float64 [...][3] (b, g, r)."""
    b = 128 + 50 * np.sin(40 * X + 1) + 40 * np.cos(33 * Y)
    g = 128 + 60 * np.sin(28 * (X + Y)) + 30 * np.cos(45 * (X - Y) + 2)
    r = 120 + 50 * np.cos(38 * X - 0.5) * np.sin(30 * Y + 0.3) + 200 * (Z0 - Z)
    return np.stack([b, g, r], -1)


def image_of(pose, disp, cam=CAM):
    """The texture at the world points the pixels of `disp` (a render at `pose`) see, float32 [rows][cols][3]; zeros where the map
    has no value."""
    fx, fy, cx, cy, baseline = (np.float64(v) for v in cam)
    rows, cols = disp.shape
    R = np.asarray(pose[0], np.float64).reshape(3, 3)
    c = -(R.T @ np.asarray(pose[1], np.float64))
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    wd = np.stack(np.broadcast_arrays((x - cx) / fx, (y - cy) / fy, np.ones((rows, cols))), -1) @ R
    with np.errstate(divide="ignore"):
        s = (fx * baseline) / disp.astype(np.float64)
    W = c + np.where(disp > 0, s, 0.0)[..., None] * wd
    return np.where((disp > 0)[..., None], texture(W[..., 0], W[..., 1], W[..., 2]), 0.0).astype(np.float32)


def flat_normals(disp):
    n = np.zeros(disp.shape + (3,), np.float32)
    n[..., 2] = -1
    return n


@functools.lru_cache(maxsize=None)
def view(scene, pose_key=None):
    """(disparity, normals, image) of `scene` ("plane" or "pyramid") at the identity, or at one of test_reproject's motions."""
    pose = IDENT if pose_key is None else motions(CAM, Z0)[pose_key]
    d = render_plane(pose) if scene == "plane" else TA.render(pose)
    n = flat_normals(d) if scene == "plane" else TA.fit_normals(d)
    return d, n, image_of(pose, d)


def neighbour_step(L):
    """The largest difference between two neighbouring finite taps of a luma plane, in levels per pixel."""
    return float(max(np.nanmax(np.abs(np.diff(L.astype(np.float64), axis=0))), np.nanmax(np.abs(np.diff(L.astype(np.float64), axis=1)))))


MOTION_NAMES = ("baseline", "advance", "yaw", "roll")


@functools.lru_cache(maxsize=None)
def degenerate():
    """name -> (guess error, reached error, info, the geometric loop's info and motion) on the plane-only scene."""
    dm, nm, im = view("plane")
    out = {}
    for name in MOTION_NAMES:
        truth = motions(CAM, Z0)[name]
        guess = perturbed(truth)
        dn, _, inew = view("plane", name)
        est, info = AP.align_color(CAM, OPT, guess, dm, nm, im, dn, inew)
        gest, ginfo = AR.align(CAM, GEO_OPT, guess, dm, nm, dn)
        out[name] = (motion_error(guess, truth), motion_error(est, truth), info, ginfo, gest, guess)
    return out


CHAIN_POSES = 6
NOISE_PX, NOISE_LEVELS, BAND = 0.3, 10.0, 0.5


def chain_pose(k):
    """Camera centre at (6k, 3k, 0) mm, rolled by 0.6k degrees about z."""
    R = rotation((0, 0, 1), 0.6 * k).T
    return R.ravel(), -(R @ np.array([0.006 * k, 0.003 * k, 0.0]))


@functools.lru_cache(maxsize=None)
def chain(scene, noisy):
    """Six poses; each frame aligned from the identity against tsdf_ref.raycast + tsdf_color_ref.color_map at the previous
    estimated pose, then integrated with colour (band 0.5) at its estimated pose -- once with the coloured loop, once with the
    geometric loop alone on the same frames."""
    rng = np.random.default_rng(21)
    poses = [chain_pose(k) for k in range(CHAIN_POSES)]
    frames = []
    for p in poses:
        d = render_plane(p) if scene == "plane" else TA.render(p)
        im = image_of(p, d)
        if noisy:
            d = np.where(d > 0, d + rng.uniform(-NOISE_PX, NOISE_PX, d.shape).astype(np.float32), d).astype(np.float32)
            im = (im + rng.uniform(-NOISE_LEVELS, NOISE_LEVELS, im.shape)).astype(np.float32)
        frames.append((d, im))
    out = {}
    for kind in ("color", "geometric"):
        first = TC.integrate(GRID, TR.clear(GRID), TC.clear(GRID), frames[0][0], frames[0][1], CAM, *poses[0], band=BAND)
        vol, col = first["voxels"], first["colors"]
        pose, valid, used = poses[0], [], []
        for k in range(1, CHAIN_POSES):
            ray = TR.raycast(GRID, vol, CAM, pose[0], pose[1], ROWS, COLS, **RAY)
            if kind == "color":
                model = TC.color_map(GRID, col, ray["disp"], CAM, pose[0], pose[1])["bgr"]
                M, info = AP.align_color(CAM, OPT, IDENT, ray["disp"], ray["normals"], model, *frames[k])
                valid.append(info["geo"]["valid"])
                used.append(info["n_photo_used"])
            else:
                M, info = AR.align(CAM, GEO_OPT, IDENT, ray["disp"], ray["normals"], frames[k][0])
                valid.append(info["valid"])
            pose = AR.compose(M, pose)
            step = TC.integrate(GRID, vol, col, frames[k][0], frames[k][1], CAM, *pose, band=BAND)
            vol, col = step["voxels"], step["colors"]
        out[kind] = dict(error=motion_error(pose, poses[-1]), valid=valid, used=used)
    out["none"] = motion_error(poses[0], poses[-1])
    return out


def profile_text():
    """The text of profiles/align_color_accuracy.txt: the reached errors of the definition."""
    lines = ["# pm_align_color_disparity's definition (tests/align_photo_ref.py) on the scenes of tests/test_align_photo.py, %dx%d." % (COLS, ROWS),
             "# Degenerate scene: the plane at 2 m alone, the analytic texture, noiseless float images, lambda %.2f, huber_levels %.0f." % (LAMBDA, HUBER_LEVELS),
             "# The guess is the truth turned by %.1f degrees about (1, 1, 1) and moved by %.0f mm along each axis; the geometric loop" % (
                 TA.PERTURB_DEG, 1e3 * TA.PERTURB_M),
             "# alone returns valid == 0 and the guess.  Written by `python tests/test_align_photo.py`; the test asserts twice the reached",
             "# values below.",
             "# motion     guess: deg  metres    reached: deg  metres    iterations  photo used  rms_levels"]
    for name, (g, r, info, *_) in degenerate().items():
        lines.append("motion %-9s guess %.6f %.6f reached %.6f %.6f iterations %d used %d rms_levels %.6f" % (
            name, g[0], g[1], r[0], r[1], info["geo"]["iterations"], info["n_photo_used"], info["rms_levels"]))
    lines += ["# Chains: six poses, camera centre at (6k, 3k, 0) mm, rolled 0.6k degrees; each frame from the identity against the raycast and",
              "# colour map of the model at the previous estimated pose.  noisy: U(-%.1f, %.1f) px and U(-%.0f, %.0f) levels.  The pose error of"
              % (NOISE_PX, NOISE_PX, NOISE_LEVELS, NOISE_LEVELS),
              "# the LAST frame; `valid`: the steps whose answer was flagged valid.  A record; the test asserts only what its docstring says.",
              "# On the pyramid the model's colour is a trilinear mean over 1 cm voxels (two pixels): it is smoother than the frames, and",
              "# where geometry alone constrains the pose the photometric term can make the chain worse."]
    for scene in ("plane", "pyramid"):
        for noisy in (False, True):
            c = chain(scene, noisy)
            for kind in ("color", "geometric"):
                lines.append("chain %-7s %-9s %-9s %.6f deg %.6f m valid %d/%d" % (
                    scene, "noisy" if noisy else "noiseless", kind, *c[kind]["error"], sum(c[kind]["valid"]), CHAIN_POSES - 1))
            lines.append("chain %-7s %-9s %-9s %.6f deg %.6f m" % (scene, "noisy" if noisy else "noiseless", "no-motion", *c["none"]))
    return "\n".join(lines) + "\n"


def profile_values():
    out = {}
    for line in open(PROFILE):
        m = re.match(r"motion (\w+)\s+guess \S+ \S+ reached (\S+) (\S+)", line)
        if m:
            out[m.group(1)] = (float(m.group(2)), float(m.group(3)))
    return out


# ---- 1. the definition ----------------------------------------------------------------------------------------------------------
SPECIAL_CHANNELS = np.array([np.nan, np.inf, -np.inf], np.float32)


def test_luma_of_bytes_floats_specials_and_zeros():
    rng = np.random.default_rng(1)
    b8 = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
    b8[0, 0] = 0
    b8[0, 1] = (0, 0, 1)
    f = b8.astype(np.float32)
    for zero in (False, True):
        L8, Lf = AP.luma(b8, zero), AP.luma(f, zero)
        assert np.array_equal(bits(L8), bits(Lf))
        want = np.float32(np.float32(np.float32(f[2, 3, 0] * np.float32(0.114)) + np.float32(f[2, 3, 1] * np.float32(0.587))) + np.float32(f[2, 3, 2] * np.float32(0.299)))
        assert L8[2, 3] == want
        assert np.isnan(L8[0, 0]) == zero and (zero or L8[0, 0] == 0) and L8[0, 1] == np.float32(0.299)
        assert np.isfinite(L8).sum() == L8.size - int(zero)
    g = f.copy()
    g[1, 1, 0], g[1, 2, 1], g[1, 3, 2] = SPECIAL_CHANNELS
    g[2, 2] = (-0.0, 0.0, -0.0)
    g[2, 4] = (-5.0, 3e38, 1e-45)
    for zero in (False, True):
        L = AP.luma(g, zero)
        nan = np.isnan(L)
        assert nan[1, 1] and nan[1, 2] and nan[1, 3] and nan[2, 2] == zero and np.isfinite(L[2, 4])
        assert (bits(L[nan]) == 0x7FC00000).all() and nan.sum() == 3 + 2 * int(zero)


def test_constant_images_add_nothing():
    """Every tap equal: dt = db = 0, top = bot = L, val = L + (b * 0) = L, gx = gy = 0, r = L - L = 0: every J is (+-)0, H and g of
    the photometric record are 0, the blend equals the geometric record numerically and the coloured loop returns align_ref.align's
    motion bit for bit.  The same holds with lambda = 0 on textured images."""
    dm, nm, _ = view("pyramid")
    truth = motions(CAM, Z0)["yaw"]
    dn = TA.render(truth)
    flat = np.full((ROWS, COLS, 3), 77.0, np.float32)
    lum = AP.luma(flat, True)
    pe = AP.evaluate(CAM, PHOTO_OPT, truth, dm, lum, dn, lum)
    assert pe["n_used"] > 0.5 * ROWS * COLS and (pe["residual"] == 0).all() and (pe["gradient"] == 0).all()
    assert (pe["H"] == 0).all() and (pe["g"] == 0).all() and pe["rr"] == 0
    ge = AR.evaluate(CAM, GEO_OPT, truth, dm, nm, dn)
    both = AP.blend(ge, pe, LAMBDA)
    assert np.array_equal(both["H"], ge["H"]) and np.array_equal(both["g"], ge["g"]) and both["rr"] == ge["rr"]
    assert both["n_used"] == ge["n_used"] + pe["n_used"]
    guess = perturbed(truth)
    want, winfo = AR.align(CAM, GEO_OPT, guess, dm, nm, dn)
    _, _, im = view("pyramid")
    inew = image_of(truth, dn)
    for opt, model, new in ((OPT, flat, flat), (dict(OPT, lam=0.0), im, inew), (OPT, flat, np.full((ROWS, COLS, 3), 77, np.uint8))):
        got, info = AP.align_color(CAM, opt, guess, dm, nm, model, dn, new)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
        assert info["geo"]["iterations"] == winfo["iterations"] and info["geo"]["valid"] == 1
        assert np.array_equal(bits(info["geo"]["H"]), bits(winfo["H"])) and bits(np.float64(info["geo"]["rms_px"])) == bits(np.float64(winfo["rms_px"]))
        assert np.array_equal(info["H"], winfo["H"])
    assert info["rms_levels"] == 0 and info["n_photo_used"] > 0.5 * ROWS * COLS  # (the last case: constant images)


def photo_class_cases():
    """(name, motion, Dm, Lm, Dn, Ln, options) on a 6x9 map of one plane; each produces the class(es) its name says."""
    rows, cols = 6, 9
    cam = (30.0, 28.0, 4.2, 2.6, 0.1)
    d0 = np.float32(cam[0] * cam[4] / 1.5)
    Dm = np.full((rows, cols), d0, np.float32)
    yy, xx = np.mgrid[:rows, :cols]
    Lm = (100 + 7 * xx + 3 * yy).astype(np.float32)
    opt = AP.photo_options(max_diff=0.6, huber_levels=6.0)
    shift = (I3, np.array([0.3 * 1.5 / cam[0], 0.6 * 1.5 / cam[1], 0.0]))  # u = x + 0.3, v = y + 0.6: no rounding puts u on x
    cases = {}
    Ln = Lm + np.where(xx % 2, np.float32(5.0), np.float32(0.5))
    cases["used, both Huber branches"] = (shift, Dm, Lm, Dm, Ln.astype(np.float32), opt)
    cases["behind the camera"] = ((I3, np.array([0.0, 0.0, -10.0])), Dm, Lm, Dm, Lm, opt)
    cases["outside the image"] = ((I3, np.array([100.0, 0.0, 0.0])), Dm, Lm, Dm, Lm, opt)
    cases["the cell at the last column and row"] = (shift, Dm, Lm, Dm, Lm, opt)
    Dn = Dm.copy()
    Dn[1, :4] = (0.0, -0.0, np.nan, -3.0)  # (iu, iv) = (x, y + 1): read by the model pixels of row 0
    Dn[2, 0] = d0 + 5  # an occluder in front of the model
    Dn[2, 1] = d0 - 1  # the model in front of what the frame sees
    Ln2 = Lm.copy()
    Ln2[3, 3] = np.nan   # a tap of the cells of (2, 2), (2, 3), (3, 2) and (3, 3)
    Ln2[5, 6] = np.inf
    cases["unmeasured and gated"] = (shift, Dm, Lm, Dn, Ln2, opt)
    Dm2, Lm2 = Dm.copy(), Lm.copy()
    Dm2[2, :3] = (0.0, np.nan, -1.0)
    Lm2[3, :3] = (np.nan, np.inf, -np.inf)  # a model pixel without colour
    cases["no model"] = (shift, Dm2, Lm2, Dm, Lm, opt)
    cases["min_disp"] = (shift, Dm, Lm, Dm, Lm, dict(opt, min_disp=float(d0) + 1))
    return cam, cases


def test_every_class_is_produced_and_every_branch_is_reached():
    cam, cases = photo_class_cases()
    seen, weights = set(), set()
    for name, (motion, Dm, Lm, Dn, Ln, opt) in cases.items():
        ev = AP.evaluate(cam, opt, motion, Dm, Lm, Dn, Ln)
        c = ev["cls"]
        rows, cols = c.shape
        seen |= set(int(v) for v in np.unique(c))
        assert ev["n_model"] == (c != 0).sum() and ev["n_gate"] == (c >= 3).sum() and ev["n_used"] == (c == 4).sum()
        assert (ev["residual"][c != AP.USED] == 0).all() and not np.signbit(ev["residual"][c != AP.USED]).any()
        inner = np.zeros_like(c, bool)
        inner[:rows - 1, :cols - 1] = True  # x0 = x, y0 = y under `shift`: the cell of the last column or row leaves the image
        if name == "used, both Huber branches":
            assert (c[inner] == AP.USED).all() and (c[~inner] == AP.OUTSIDE).all()
            r = np.abs(ev["residual"][inner].astype(np.float64))
            weights |= {"one" if v <= opt["huber_levels"] else "less" for v in r}
        if name in ("behind the camera", "outside the image"):
            assert (c == AP.OUTSIDE).all() and ev["n_gate"] == 0
        if name == "the cell at the last column and row":
            # (x, y) = (cols - 2, rows - 2) reads the taps of the last column and the last row and is USED; one further is OUTSIDE
            assert c[rows - 2, cols - 2] == AP.USED and (c[rows - 1] == AP.OUTSIDE).all() and (c[:, cols - 1] == AP.OUTSIDE).all()
            # the plane 100 + 7x + 3y is linear: the bilinear value is exact up to rounding, the gradient is (7, 3)
            assert np.abs(ev["residual"][inner] - (7 * 0.3 + 3 * 0.6)).max() < 1e-4
            assert np.abs(ev["gradient"][inner] - (7, 3)).max() < 1e-9
        if name == "unmeasured and gated":
            # the projection (x + 0.3, y + 0.6) rounds to (x, y + 1): the new map is read one row below, the cell starts at (x, y)
            assert (c[0, :4] == AP.UNMEASURED).all() and (c[1, :2] == AP.GATED).all()
            for y, x in ((2, 2), (2, 3), (3, 2), (3, 3), (4, 5), (4, 6)):  # the cells with the NaN tap and with the infinite one
                assert c[y, x] == AP.UNMEASURED, (y, x)
            assert (c == AP.UNMEASURED).sum() == 10 and (c == AP.GATED).sum() == 2
            assert (c[inner] >= AP.UNMEASURED).all() and (c[~inner] == AP.OUTSIDE).all()
        if name == "no model":
            assert (c[2, :3] == AP.NO_MODEL).all() and (c[3, :3] == AP.NO_MODEL).all() and (c == AP.NO_MODEL).sum() == 6
        if name == "min_disp":
            assert (c == AP.NO_MODEL).all() and (ev["H"] == 0).all()
    assert seen == {0, 1, 2, 3, 4} and weights == {"one", "less"}
    # an image of one row or one column has no cell: nothing is USED
    for shape in ((1, 7), (7, 1), (1, 1)):
        one = np.full(shape, 2.0, np.float32)
        ev = AP.evaluate((30.0, 28.0, shape[1] / 2, shape[0] / 2, 0.1), AP.photo_options(), IDENT, one, one, one, one)
        assert (ev["cls"] == AP.OUTSIDE).all() and ev["n_used"] == 0 and ev["n_model"] == one.size


def seeded_record(pm, rng):
    H, g = TA.seeded_sums(rng)
    return pm.align_sums(H, g, float(rng.uniform(0, 9)), *(int(v) for v in rng.integers(0, 5000, 3)))


def test_blend_equals_the_reference_aliased_and_not(pm):
    rng = np.random.default_rng(8)
    lib = pm.load()
    for k in range(20):
        geo, photo = seeded_record(pm, rng), seeded_record(pm, rng)
        lam = float(rng.choice([0.0, 0.03, 1.0, 17.5]))
        want = AP.blend(geo.as_dict(), photo.as_dict(), lam)
        record = np.frombuffer(bytes(pm.align_sums(want["H"], want["g"], want["rr"], want["n_model"], want["n_gate"], want["n_used"])), np.uint8)
        out = (None, geo, photo)[k % 3]  # a fresh record, out == geo, out == photo
        got = pm.align_sums_blend(geo, photo, lam, out)
        assert np.array_equal(np.frombuffer(bytes(got), np.uint8), record), k
        if lam == 0.0 and out is None:
            assert np.array_equal(got.as_dict()["H"], geo.as_dict()["H"])
    s, o = seeded_record(pm, rng), pm.PmAlignSums()
    for args in ((None, C.byref(s), 0.5, C.byref(o)), (C.byref(s), None, 0.5, C.byref(o)), (C.byref(s), C.byref(s), 0.5, None),
                 (C.byref(s), C.byref(s), -0.5, C.byref(o)), (C.byref(s), C.byref(s), float("nan"), C.byref(o)),
                 (C.byref(s), C.byref(s), float("inf"), C.byref(o))):
        assert lib.pm_align_sums_blend(*args) == pm.PM_ERR_INVALID_ARG
    assert lib.pm_align_sums_blend(C.byref(s), C.byref(s), 0.5, C.byref(o)) == pm.PM_OK


def test_a_frame_against_itself_from_the_identity():
    """R = I, t = 0: Q == P bit for bit (tests/test_align.py), so the geometric residuals are exact zeros.  Photometrically
    u = fl(fl(fx * fl(X / Z)) + cx) with X = fl(fl((x - cx) * Z) / fx): four roundings on (x - cx) and one on the sum, so with
    eps = 2^-53, |x - cx| <= 41 and |u| <= 80:  |u - x| <= 4 eps * 41 + eps * 80 < 3e-14 pixels, likewise in v.  u may fall a hair
    BELOW x, then the cell is the one to the left and a = 1 - (a hair); the bilinear interpolant is continuous, so either way
    val differs from the tap L(y, x) by at most (|u - x| + |v - y|) * G, G the largest step between neighbouring taps, plus the
    roundings of the six operations of `sample` on values below 2 * 255: < 6 * 510 * eps < 4e-13.  So |r| <= 6e-14 * G + 4e-13
    =: B for every pixel, and rms_levels <= B.
    The first update: w = 1 (B << huber), g_j = sum_p J_pj r_p, so |g_j| <= B * sum_p |J_pj| <= B * sqrt(n * Hp_jj) by
    Cauchy-Schwarz, Hp the photometric matrix; the blended g is lambda^2 g (the geometric g is exactly 0).  delta = -H^-1 g gives
    |delta|_2 <= |g|_2 / lambda_min(H), H the blended matrix.  Each further update starts from residuals that are these roundings
    plus J * (the motion so far), which Gauss-Newton removes up to second order (1e-24): every update obeys the same bound, and
    the returned rotation (radians) and translation are each within iterations * 2 |delta|_2 (Cayley: the angle is 2 atan(|omega|/2)
    <= |omega|, the translation moves by at most |upsilon| + |omega| |t|)."""
    dm, nm, im = view("plane")
    lum = AP.luma(im, False)
    pe = AP.evaluate(CAM, PHOTO_OPT, IDENT, dm, lum, dm, lum)
    G = neighbour_step(lum)
    B = 6e-14 * G + 4e-13
    print("G", G, "B", B, "largest |r|", np.abs(pe["residual"]).max(), "used", pe["n_used"])
    assert pe["n_used"] >= (ROWS - 1) * (COLS - 1) - ROWS - COLS and 5 < G < 60
    assert np.abs(pe["residual"].astype(np.float64)).max() <= B
    (R, t), info = AP.align_color(CAM, OPT, IDENT, dm, nm, im, dm, im)
    assert info["geo"]["valid"] == 1 and info["rms_levels"] <= B and info["geo"]["rms_px"] <= 1e-9
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = info["H"]
    H = H + np.triu(H, 1).T
    Hp = np.zeros((6, 6))
    Hp[np.triu_indices(6)] = pe["H"]
    g_bound = LAMBDA ** 2 * B * np.sqrt(pe["n_used"] * np.diag(Hp))
    delta_bound = np.linalg.norm(g_bound) / np.linalg.eigvalsh(H)[0]
    err = motion_error((R, t), IDENT)
    print("delta bound", delta_bound, "iterations", info["geo"]["iterations"], "reached", err)
    assert delta_bound < 1e-9
    assert np.radians(err[0]) <= 2 * info["geo"]["iterations"] * delta_bound + 1e-15 and err[1] <= 2 * info["geo"]["iterations"] * delta_bound


@pytest.mark.parametrize("name", MOTION_NAMES)
def test_the_degenerate_plane_is_solved_with_colour(name):
    """The plane at 2 m alone: align_ref.align returns valid == 0 and the guess (its third pivot is 0, or not > 0); the coloured loop
    is valid, uses at least half of the 3840 pixels photometrically, ends nearer the truth than the guess in rotation and in
    translation, and within TWICE the values profiles/align_color_accuracy.txt records (tests/test_align.py's convention: the
    slack covers the scene generator's libm)."""
    guess_err, reached, info, ginfo, gest, guess = degenerate()[name]
    recorded = profile_values()[name]
    print(name, "guess", guess_err, "reached", reached, "recorded", recorded, "iterations", info["geo"]["iterations"], "photo used", info["n_photo_used"])
    assert ginfo["valid"] == 0 and np.array_equal(gest[0], guess[0]) and np.array_equal(gest[1], guess[1])
    assert info["geo"]["valid"] == 1 and info["n_photo_used"] >= ROWS * COLS // 2
    assert reached[0] < guess_err[0] and reached[1] < guess_err[1]
    assert reached[0] <= 2 * recorded[0] and reached[1] <= 2 * recorded[1]


@pytest.mark.parametrize("noisy", [False, True], ids=["noiseless", "noisy"])
def test_the_coloured_chain_tracks_the_plane(noisy):
    """Six poses over the plane.  The coloured chain is valid at every step and ends better than assuming no motion, in rotation
    and in translation, noiseless and with U(-0.3, 0.3) px and U(-10, 10) levels of noise; on the noiseless plane the geometric
    chain is invalid at every step.  How the two compare on the noisy plane and on the pyramid is a record in the profile."""
    c = chain("plane", noisy)
    print("noisy" if noisy else "noiseless", "colour", c["color"], "geometric", c["geometric"], "no motion", c["none"])
    assert all(c["color"]["valid"])
    assert c["color"]["error"][0] < c["none"][0] and c["color"]["error"][1] < c["none"][1]
    if not noisy:
        assert not any(c["geometric"]["valid"])


def test_the_profile_records_every_motion_and_chain():
    assert set(profile_values()) == set(MOTION_NAMES)
    text = open(PROFILE).read()
    for scene in ("plane", "pyramid"):
        for leg in ("noiseless", "noisy"):
            for kind in ("color", "geometric", "no-motion"):
                assert re.search(r"chain %s\s+%s\s+%s" % (scene, leg, kind), text), (scene, leg, kind)


# ---- 2. the kernels' code on the host -----------------------------------------------------------------------------------------------
SHAPES = {"1x1": (1, 1), "1x7": (1, 7), "2x2": (2, 2), "2x63": (2, 63), "2x64": (2, 64), "2x65": (2, 65), "1x65": (1, 65),
          "3x130": (3, 130), "5x64": (5, 64), "37x53": (37, 53)}
MOTIONS = TA.MOTIONS
KINDS = ("noise", "constants", "specials")
OUTPUTS = FA.OUTPUTS


def random_image(rng, rows, cols, special=0.0):
    """A smooth random texture with a little noise, float32 [rows][cols][3] in levels; `special` of the channels NaN or infinite
    and as many pixels all zero."""
    yy, xx = np.mgrid[:rows, :cols].astype(np.float64)
    im = np.stack([128 + 60 * np.sin(rng.uniform(0.2, 0.6) * xx + rng.uniform(0, 6)) * np.cos(rng.uniform(0.2, 0.6) * yy + rng.uniform(0, 6))
                   for _ in range(3)], -1)
    im = (im + rng.uniform(-3, 3, im.shape)).astype(np.float32)
    pick = rng.random(im.shape) < special
    im[pick] = rng.choice(SPECIAL_CHANNELS, int(pick.sum()))
    im[rng.random((rows, cols)) < special] = 0.0
    return im


@functools.lru_cache(maxsize=None)
def photo_case(shape_name, motion_name, kind):
    """A fixed case: dict(cam, opt, motion, dm, dn, bgr_model, bgr_new (float32), bgr8 (uint8), lm, ln, l8 (the lumas: the model's
    and the bytes' with zero_is_absent, the new image's without), ev (the definition's evaluation of the float images))."""
    if shape_name == "scene":
        dm, _, bgr_model = view("pyramid")
        truth = motions(CAM, Z0)["yaw"] if motion_name == "identity" else TA.case_motion(motion_name, Z0)
        dn = TA.render(truth)
        bgr_new = image_of(truth, dn)
        rng = np.random.default_rng(3)
        if kind == "specials":
            dn, bgr_new, bgr_model = dn.copy(), bgr_new.copy(), bgr_model.copy()
            dn[::5, ::7] = FA.SPECIALS[np.arange(dn[::5, ::7].size) % len(FA.SPECIALS)].reshape(dn[::5, ::7].shape)
            bgr_new[2::7, 3::5, 1] = np.nan
            bgr_model[1::6, 2::9] = 0.0
        elif kind == "noise":
            dn = (dn + rng.uniform(-0.3, 0.3, dn.shape)).astype(np.float32)
            bgr_new = (bgr_new + rng.uniform(-10, 10, bgr_new.shape)).astype(np.float32)
        cam, opt, motion = CAM, PHOTO_OPT, TA.case_motion(motion_name, Z0)
    else:
        rows, cols = shape = SHAPES[shape_name]
        cam = TA.case_camera(shape)
        depth = 1.5
        mid = cam[0] * cam[4] / depth
        rng = np.random.default_rng(sum(map(ord, shape_name + motion_name + kind)) + 1000)
        if kind == "constants":
            dm = np.full(shape, mid, np.float32)
            dn = np.full(shape, mid * 1.01, np.float32)
            bgr_model = np.full(shape + (3,), 90.0, np.float32)
            bgr_new = np.full(shape + (3,), 97.5, np.float32)
        else:
            special = 0.15 if kind == "specials" else 0.0
            valid = 1.0 if kind == "noise" else 0.8
            dm = FA.random_disp(rng, rows, cols, valid=valid, special=special, lo=0.95 * mid, hi=1.05 * mid)
            dn = FA.random_disp(rng, rows, cols, valid=valid, special=special, lo=0.95 * mid, hi=1.05 * mid)
            bgr_model = random_image(rng, rows, cols, special / 3)
            bgr_new = random_image(rng, rows, cols, special / 3)
        opt = AP.photo_options(max_diff=0.06 * mid, huber_levels=25.0)
        motion = TA.case_motion(motion_name, depth)
    with np.errstate(invalid="ignore"):
        bgr8 = np.clip(np.rint(np.nan_to_num(bgr_new, nan=0.0, posinf=255.0, neginf=0.0)), 0, 255).astype(np.uint8)
    lm, ln, l8 = AP.luma(bgr_model, True), AP.luma(bgr_new, False), AP.luma(bgr8, True)
    return dict(cam=cam, opt=opt, motion=motion, dm=dm, dn=dn, bgr_model=bgr_model, bgr_new=bgr_new, bgr8=bgr8, lm=lm, ln=ln, l8=l8,
                ev=AP.evaluate(cam, opt, motion, dm, lm, dn, ln))


def test_conditions_the_cases_use_gate_and_drop_pixels():
    """The fixed cases are not empty: pixels are used under the identity, the yaw and the roll in every kind of map, both Huber
    branches and every class occur, the motions behind and beside the scene use nothing, and an image without a cell uses nothing."""
    classes = set()
    for shape in ("37x53", "3x130", "scene", "2x2"):
        for motion in MOTIONS:
            for kind in KINDS:
                ev = photo_case(shape, motion, kind)["ev"]
                classes |= set(int(v) for v in np.unique(ev["cls"]))
                if motion in ("behind", "beside"):
                    assert (ev["n_used"] == 0 or kind == "specials") and ev["n_model"] > 0, (shape, motion, kind)
                elif shape != "2x2":
                    assert ev["n_used"] > 5 and ev["rr"] > 0, (shape, motion, kind, ev["n_used"])
    assert classes == {0, 1, 2, 3, 4}
    assert photo_case("2x2", "identity", "constants")["ev"]["n_used"] == 1 and photo_case("2x2", "yaw", "noise")["ev"]["n_used"] == 1
    for shape in ("2x63", "2x64", "2x65"):  # one row of cells across the chunk edge
        assert photo_case(shape, "identity", "constants")["ev"]["n_used"] == SHAPES[shape][1] - 1
    for shape in ("1x1", "1x7", "1x65"):
        ev = photo_case(shape, "identity", "noise")["ev"]
        assert ev["n_used"] == 0 and (ev["cls"] == AP.OUTSIDE).all()
    c = photo_case("37x53", "yaw", "noise")
    r = np.abs(c["ev"]["residual"][c["ev"]["cls"] == AP.USED])
    assert (r <= c["opt"]["huber_levels"]).any() and (r > c["opt"]["huber_levels"]).any()


@pytest.fixture(scope="module")
def host_photo_exe(tmp_path_factory):
    """tests/cpp/align_photo_host_main.cpp: csrc/pm_align_photo_body.hpp compiled for the host alone, with the sanitizers."""
    return build_host_kernel(tmp_path_factory.mktemp("alignphotohost") / "align_photo_host_main", "align_photo_host_main.cpp")


def _dump_case(path, c):
    opt, motion, ev = c["opt"], c["motion"], c["ev"]
    dump_case(path, [*c["cam"], *c["dm"].shape, opt["min_disp"], opt["max_diff"], opt["huber_levels"], *np.asarray(motion[0]).ravel(), *motion[1]],
              disp_model=c["dm"], disp_new=c["dn"], bgr_model=c["bgr_model"], bgr_new=c["bgr_new"], bgr8=c["bgr8"],
              want_luma_model=c["lm"], want_luma_new=c["ln"], want_luma8=c["l8"], want_record=AR.record(ev), want_class=ev["cls"],
              want_residual=ev["residual"])


def test_kernel_code_on_the_host_equals_the_definition(host_photo_exe, tmp_path):
    """pm_align_photo_body.hpp composed serially in the kernels' layout over 2x2, 1x65, 5x64, 3x130 and 37x53, blocks and threads
    forwards and backwards, each optional plane alone and neither: the three luma planes, the 240-byte record, the classes and
    the residuals equal the .npy dumps of the definition byte for byte, and AddressSanitizer / UBSan see every access into
    buffers of exactly the size the stage may touch."""
    used, k = 0, 0
    for shape in ("2x2", "1x65", "5x64", "3x130", "37x53"):
        for motion in MOTIONS:
            c = photo_case(shape, motion, KINDS[k % 3])
            d = str(tmp_path / ("case%d" % k))
            _dump_case(d, c)
            r = subprocess.run([host_photo_exe, d], capture_output=True, text=True)
            assert r.returncode == 0, (shape, motion, KINDS[k % 3], r.stderr[-3000:])
            used += c["ev"]["n_used"]
            k += 1
    assert used > 2000
    c = photo_case("37x53", "roll", "noise")
    d = str(tmp_path / "flip")
    _dump_case(d, c)
    assert c["ev"]["n_used"] > 500
    assert_program_compares(host_photo_exe, d, [("want_record", np.uint8, "the record differs"), ("want_class", np.uint8, "the classes differ"),
                                                ("want_residual", np.uint32, "the residuals differ"),
                                                ("want_luma_model", np.uint32, "the model luma differs"),
                                                ("want_luma_new", np.uint32, "the new luma differs"),
                                                ("want_luma8", np.uint32, "the luma of bytes differs")])


def test_headers_declare_and_the_library_exports_the_photometric_functions(pm):
    text = open(os.path.join(ROOT, "include", "pm", "imaging.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = pm.load()
    for name in ("pm_bgr_luma", "pm_align_photo_evaluate", "pm_align_color_disparity"):
        assert re.search(r"\bint\s+%s\s*\(\s*pm_handle\s*\*" % name, text), name
    assert re.search(r"\bint\s+pm_align_sums_blend\s*\(\s*const\s+pm_align_sums\s*\*", text)
    for name in ("pm_bgr_luma", "pm_align_photo_evaluate", "pm_align_sums_blend", "pm_align_color_disparity",
                 "pm_debug_align_photo_scratch_bytes"):
        assert name in pm.EXPORTS and hasattr(lib, name), name
    for name in ("pm_align_photo_options", "pm_align_color_options", "pm_align_color_info"):
        assert "typedef struct " + name in text, name
    assert text.index("pm_tsdf_color_points") < text.index("pm_bgr_luma") < text.index("pm_device_malloc")
    assert "#define PM_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "pm", "patchmatch.h")).read() and pm.PM_ABI_VERSION == 6
    assert (C.sizeof(pm.PmAlignPhotoOptions), C.sizeof(pm.PmAlignColorOptions), C.sizeof(pm.PmAlignColorInfo)) == (16, 56, 392)
    assert C.sizeof(pm.PmAlignSums) == 240 and C.sizeof(pm.PmAlignInfo) == 200
    assert pm.align_photo_scratch_bytes(720, 1280) == 256 + 720 * 28 * 8 + 2 * 4 * 720 * 1280
    assert pm.align_photo_scratch_bytes(0, 5) == 0 and pm.align_photo_scratch_bytes(5, 0) == 0
    assert pm.align_scratch_bytes(720) == 256 + 720 * 28 * 8
    csrc = os.path.join(ROOT, "ocean-perception_amd", "csrc")
    assert '#include "pm_align_photo.hpp"' in open(os.path.join(csrc, "pm_stages.hip")).read()
    assert "pm_align_photo.hpp" in open(os.path.join(csrc, "pm_handle.hpp")).read()
    body = open(os.path.join(csrc, "pm_align_photo_body.hpp")).read()
    assert "align_terms(" in body and "align_lane_tail(" in body and "wj * J[j]" not in body  # the terms are stated once


# ---- 3. device parity ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        yield e


def upload(torch, a, offset=0):
    """`a` on the device, `offset` elements past the start of its allocation -> (tensor, address)."""
    a = np.ascontiguousarray(a).ravel()
    t = torch.zeros(a.size + offset, dtype=getattr(torch, str(a.dtype)), device="cuda")
    t[offset:] = torch.from_numpy(a)
    return t, t.data_ptr() + offset * a.dtype.itemsize


LUMA_SHAPES = ((1, 1), (1, 63), (1, 64), (1, 65), (37, 53), (9, 300))


@gpu
@pytest.mark.parametrize("shape", LUMA_SHAPES, ids=["%dx%d" % s for s in LUMA_SHAPES])
def test_bgr_luma_equals_the_definition(pm, engine, shape):
    """One pixel; the block edge (63, 64, 65 pixels); rows and columns that are no multiple of the block; several blocks each way:
    bytes and floats with NaN, infinities, negative zeros and all-zero pixels, both settings of zero_is_absent, the inputs 1, 2
    and 3 elements past a 16-byte boundary and the output as many floats: the plane's bits, guards intact, inputs untouched."""
    import torch
    rows, cols = shape
    rng = np.random.default_rng(rows * 1000 + cols)
    f = random_image(rng, rows, cols, 0.1)
    f[rng.random((rows, cols)) < 0.05] = (-0.0, 0.0, -0.0)
    b8 = rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8)
    b8[rng.random((rows, cols)) < 0.2] = 0
    k = 0
    for image in (f, b8):
        for zero in (False, True):
            off = k % 4
            t, ptr = upload(torch, image, off)
            out = FA.Guarded(torch, 4 * rows * cols, 4 * off)
            torch.cuda.synchronize()
            engine.bgr_luma(rows, cols, out.ptr, d_bgr8=ptr if image.dtype == np.uint8 else None,
                            d_bgr=ptr if image.dtype != np.uint8 else None, zero_is_absent=zero)
            engine.synchronize()
            got, want = out.read(np.float32).reshape(rows, cols), AP.luma(image, zero)
            bad = np.argwhere(bits(got) != bits(want))
            assert len(bad) == 0, (shape, image.dtype, zero, [(int(y), int(x), got[y, x], want[y, x]) for y, x in bad[:6]])
            assert np.array_equal(t.cpu().numpy()[off:].view(np.uint8), image.ravel().view(np.uint8))
            k += 1


def check_photo(torch, e, c, outputs=OUTPUTS, offset_floats=0):
    """One pm_align_photo_evaluate call against the definition, as fuzz_align.check_align."""
    rows, cols = c["dm"].shape
    want, off = c["ev"], 4 * offset_floats
    ins = [upload(torch, c[k], offset_floats) for k in ("dm", "lm", "dn", "ln")]
    cls = FA.Guarded(torch, rows * cols, offset_floats) if "class" in outputs else None
    res = FA.Guarded(torch, 4 * rows * cols, off) if "residual" in outputs else None
    dev = FA.Guarded(torch, 240) if "d_sums" in outputs else None
    torch.cuda.synchronize()
    sums = e.align_photo_evaluate(c["cam"], ins[0][1], ins[1][1], ins[2][1], ins[3][1], rows, cols, c["motion"], c["opt"],
                                  cls.ptr if cls else None, res.ptr if res else None, dev.ptr if dev else None, "sums" in outputs)
    e.synchronize()
    record = AR.record(want)

    def same_record(got, where):
        bad = np.flatnonzero(got.view(np.uint64) != record.view(np.uint64))
        assert len(bad) == 0, "the %s record differs in doubles %s; (got, want): %s" % (
            where, bad[:6], [(got.view(np.float64)[i], record.view(np.float64)[i]) for i in bad[:6]])

    if "sums" in outputs:
        same_record(np.frombuffer(bytes(sums), np.uint8), "host")
    else:
        assert sums is None
    if dev:
        same_record(dev.read(np.uint8), "device")
    if cls:
        got = cls.read(np.uint8).reshape(rows, cols)
        bad = np.argwhere(got != want["cls"])
        assert len(bad) == 0, "%d classes differ; (y, x, got, want): %s" % (
            len(bad), [(int(y), int(x), int(got[y, x]), int(want["cls"][y, x])) for y, x in bad[:6]])
    if res:
        got = res.read(np.float32).reshape(rows, cols)
        bad = np.argwhere(bits(got) != bits(want["residual"]))
        assert len(bad) == 0, "%d residuals differ; (y, x, got, want): %s" % (
            len(bad), [(int(y), int(x), float(got[y, x]), float(want["residual"][y, x])) for y, x in bad[:6]])
    for (t, _), k in zip(ins, ("dm", "lm", "dn", "ln")):
        assert np.array_equal(bits(t.cpu().numpy()[offset_floats:]), bits(c[k]).ravel()), "the call wrote to " + k


EVALUATE_SHAPES = ["1x1", "1x7", "2x2", "2x63", "2x64", "2x65", "3x130", "5x64", "37x53", "scene"]


@gpu
@pytest.mark.parametrize("shape", EVALUATE_SHAPES)
def test_align_photo_evaluate_equals_the_definition(pm, engine, shape):
    """No cell at all (1x1, 1x7: every model pixel OUTSIDE); one cell; the chunk edge with one row of cells (63, 64, 65 pixels);
    three chunks per lane sum; rows beyond one block; a map that is no multiple of anything; the 48x80 scene -- each under the
    identity, a yaw, a roll and motions that put the model behind and beside the camera, with images from noise, constants and
    NaN lumas with special disparities, the inputs 4, 8 and 12 bytes past a 16-byte boundary in turn: the record on the device
    and on the host, the classes and the residuals at tolerance 0."""
    import torch
    k = 0
    for motion in MOTIONS:
        for kind in KINDS:
            check_photo(torch, engine, photo_case(shape, motion, kind), offset_floats=k % 4)
            k += 1


@gpu
def test_each_output_alone_and_absent_and_two_runs_agree(pm, engine):
    import torch
    for outputs in [tuple(k for k in OUTPUTS if k != drop) for drop in OUTPUTS] + [(k,) for k in OUTPUTS]:
        check_photo(torch, engine, photo_case("37x53", "roll", "specials"), outputs=outputs)
        check_photo(torch, engine, photo_case("3x130", "yaw", "noise"), outputs=outputs, offset_floats=1)
    c = photo_case("scene", "yaw", "noise")
    t = [upload(torch, c[k])[0] for k in ("dm", "lm", "dn", "ln")]
    recs = [FA.Guarded(torch, 240) for _ in range(2)]
    torch.cuda.synchronize()
    for rec in recs:
        engine.align_photo_evaluate(c["cam"], *(x.data_ptr() for x in t), ROWS, COLS, c["motion"], c["opt"], d_sums=rec.ptr)
    engine.synchronize()
    a, b = (rec.read(np.uint8) for rec in recs)
    assert c["ev"]["n_used"] > 1000 and np.array_equal(a, b) and np.array_equal(a, AR.record(c["ev"]))


def same_color_result(got, want):
    """(R, t, info) of the device against the definition's ((R, t), info), bit for bit."""
    R, t, info = got
    (wR, wt), winfo = want
    assert np.array_equal(bits(R), bits(wR)) and np.array_equal(bits(t), bits(wt)), (R, t, wR, wt)
    for k in ("valid", "n_model", "n_gate", "n_used", "iterations"):
        assert info["geo"][k] == winfo["geo"][k], (k, info["geo"][k], winfo["geo"][k])
    for k in ("n_photo_model", "n_photo_gate", "n_photo_used"):
        assert info[k] == winfo[k], (k, info[k], winfo[k])
    for got_v, want_v in ((info["geo"]["rms_px"], winfo["geo"]["rms_px"]), (info["rms_levels"], winfo["rms_levels"])):
        assert bits(np.float64(got_v)) == bits(np.float64(want_v)), (got_v, want_v)
    assert np.array_equal(bits(info["geo"]["H"]), bits(np.asarray(winfo["geo"]["H"], np.float64)))
    assert np.array_equal(bits(info["H"]), bits(np.asarray(winfo["H"], np.float64)))


def to_bytes(image):
    return np.clip(np.rint(image), 0, 255).astype(np.uint8)


@gpu
@pytest.mark.parametrize("scene,image", [("plane", "float"), ("plane", "bytes"), ("pyramid", "float"), ("pyramid", "bytes"), ("constant", "float")])
def test_align_color_disparity_equals_the_definitions_loop(pm, engine, scene, image):
    """pm_align_color_disparity equals align_photo_ref.align_color bit for bit -- the motion and the info with both matrices: the
    degenerate plane and the pyramid under the 2-degree yaw from the perturbed guess, the new image as floats and as bytes; and
    the plane with constant images, where nothing constrains three parameters and the answer is the guess."""
    import torch
    name = "plane" if scene == "constant" else scene
    dm, nm, im = view(name)
    truth = motions(CAM, Z0)["yaw"]
    dn, _, inew = view(name, "yaw") if name == "plane" else (TA.render(truth), None, image_of(truth, TA.render(truth)))
    if scene == "constant":
        im, inew = np.full_like(im, 50.0), np.full_like(inew, 50.0)
    new = to_bytes(inew) if image == "bytes" else inew
    guess = perturbed(truth)
    want = AP.align_color(CAM, OPT, guess, dm, nm, im, dn, new)
    t = [upload(torch, a) for a in (dm, nm, im, dn, new)]
    torch.cuda.synchronize()
    got = engine.align_color_disparity(CAM, t[0][1], t[1][1], t[2][1], t[3][1], ROWS, COLS, d_bgr8_new=t[4][1] if image == "bytes" else None,
                                       d_bgr_new=t[4][1] if image != "bytes" else None, guess=guess, options=OPT)
    same_color_result(got, want)
    if scene == "constant":
        assert want[1]["geo"]["valid"] == 0 and np.array_equal(got[0], guess[0])
    else:
        assert want[1]["geo"]["valid"] == 1 and want[1]["geo"]["iterations"] > 1 and want[1]["n_photo_used"] > 1900


@gpu
def test_align_color_directly_behind_a_raycast_and_a_colour_map(pm, engine):
    """clear, integrate with colour, raycast, colour map and the coloured loop on the handle's stream with nothing copied and
    nothing synchronised in between: the motion and the info equal the definition on the definition's own render."""
    import torch
    truth = chain_pose(2)
    d0, _, im0 = view("pyramid")
    d1 = TA.render(truth)
    im1 = to_bytes(image_of(truth, d1))
    n_vox = GRID["nx"] * GRID["ny"] * GRID["nz"]
    vol, col = FA.Guarded(torch, 8 * n_vox), FA.Guarded(torch, 16 * n_vox)
    t = [upload(torch, a) for a in (d0, im0, d1, im1)]
    out, nrm, bgr = FA.Guarded(torch, 4 * ROWS * COLS), FA.Guarded(torch, 12 * ROWS * COLS), FA.Guarded(torch, 12 * ROWS * COLS)
    torch.cuda.synchronize()
    engine.tsdf_clear(GRID, vol.ptr)
    engine.tsdf_color_clear(GRID, col.ptr)
    engine.tsdf_integrate_color(CAM, GRID, IDENT, t[0][1], ROWS, COLS, vol.ptr, col.ptr, d_bgr=t[1][1], band=BAND)
    engine.tsdf_raycast(CAM, GRID, IDENT, vol.ptr, ROWS, COLS, d_disp_out=out.ptr, d_normals_out=nrm.ptr, **RAY)
    engine.tsdf_color_map(CAM, GRID, IDENT, col.ptr, out.ptr, ROWS, COLS, d_bgr_out=bgr.ptr)
    got = engine.align_color_disparity(CAM, out.ptr, nrm.ptr, bgr.ptr, t[2][1], ROWS, COLS, d_bgr8_new=t[3][1], options=OPT)
    first = TC.integrate(GRID, TR.clear(GRID), TC.clear(GRID), d0, im0, CAM, *IDENT, band=BAND)
    ray = TR.raycast(GRID, first["voxels"], CAM, *IDENT, ROWS, COLS, **RAY)
    model = TC.color_map(GRID, first["colors"], ray["disp"], CAM, *IDENT)["bgr"]
    want = AP.align_color(CAM, OPT, None, ray["disp"], ray["normals"], model, d1, im1)
    assert want[1]["geo"]["valid"] == 1 and want[1]["n_photo_used"] > 0.5 * ROWS * COLS
    same_color_result(got, want)
    assert np.array_equal(bits(bgr.read(np.float32)), bits(model).ravel())


@gpu
@pytest.mark.parametrize("mode", ["scalar", "planes"])
def test_align_color_directly_behind_a_match_on_the_handles_stream(pm, synth, mode):
    """A Match() of a synthetic pair into a device buffer, its normals by the plane fit, then the coloured loop of the map and the
    left image against themselves from a small guess, all on the handle's stream with nothing synchronised in between: the motion
    and the info equal the definition on the downloaded map and normals."""
    import torch
    rows, cols = 96, 128
    cam = (100.0, 100.0, 64.0, 48.0, 0.02)
    kw = dict(mode=pm.PM_MODE_PLANES) if mode == "planes" else {}
    p = synth.make_pair(5, rows=rows, cols=cols, n_points=40, dilate_factor=2)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    L, R, SL, SR = (up(p[k]) for k in ("left", "right", "seed_l", "seed_r"))
    bgr8 = np.repeat(np.asarray(p["left"], np.uint8)[..., None], 3, -1)
    bgr8[..., 1] //= 2
    model = bgr8.astype(np.float32)
    B8, BM = up(bgr8), up(model)
    D = torch.zeros((2, rows, cols), dtype=torch.float32, device="cuda")
    N = torch.zeros((rows, cols, 3), dtype=torch.float32, device="cuda")
    guess = (rotation((0, 1, 0), 0.3).ravel(), np.array([0.001, 0.0, 0.0]))
    opt = AP.color_options(max_diff=2.0, huber_px=0.5, min_used=6, iterations=3, huber_levels=HUBER_LEVELS, lam=LAMBDA)
    torch.cuda.synchronize()
    with pm.Engine(pm.default_params(0, patch=5, patchmatch_iters=2, max_disp=32, **kw), max_rows=rows, max_cols=cols) as e:
        e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), D[0].data_ptr(), D[1].data_ptr())
        fit = pm.PmNormalsFit(2, 1.0, 9)
        e._check(e.lib.pm_disparity_normals(e.h, pm._ref(pm.cloud_camera(cam)), C.byref(fit), D[0].data_ptr(), rows, cols,
                                            N.data_ptr(), None, None), "pm_disparity_normals")
        got = e.align_color_disparity(cam, D[0].data_ptr(), N.data_ptr(), BM.data_ptr(), D[0].data_ptr(), rows, cols,
                                      d_bgr8_new=B8.data_ptr(), guess=guess, options=opt)
    disp, normals = D[0].cpu().numpy(), N.cpu().numpy()
    want = AP.align_color(cam, opt, guess, disp, normals, model, disp, bgr8)
    print(mode, "geo used", want[1]["geo"]["n_used"], "photo used", want[1]["n_photo_used"], "iterations", want[1]["geo"]["iterations"])
    assert want[1]["n_photo_used"] > 500
    same_color_result(got, want)


@gpu
def test_invalid_arguments_are_named_in_order_and_nothing_is_enqueued(pm, engine):
    """PM_ERR_INVALID_ARG / PM_ERR_SIZE with the whole text of pm_last_error, the checks in the documented order (a call with
    fault k also has every later fault); the outputs keep their guard patterns and their payloads, the host outputs their values."""
    import torch
    rows, cols = 16, 24
    lib, h = engine.lib, engine.h
    cam = (40.0, 40.0, 12.0, 8.0, 0.1)
    disp = torch.full((rows, cols), 4.25, dtype=torch.float32, device="cuda")
    lum = torch.full((rows, cols), 80.0, dtype=torch.float32, device="cuda")
    nrm = torch.zeros((rows, cols, 3), dtype=torch.float32, device="cuda")
    nrm[..., 2] = -1
    img = torch.full((rows, cols, 3), 80.0, dtype=torch.float32, device="cuda")
    img8 = torch.full((rows, cols, 3), 80, dtype=torch.uint8, device="cuda")
    bufs = {k: FA.Guarded(torch, n) for k, n in (("cls", rows * cols), ("res", 4 * rows * cols), ("rec", 240), ("luma", 4 * rows * cols))}
    host = pm.PmAlignSums()
    host.n_used = -5
    out, info = pm.PmMotion(), pm.PmAlignColorInfo()
    out.t[0], info.n_photo_used = 7.0, -5
    nan, inf = float("nan"), float("inf")
    D, Lp, Np, Ip, I8 = disp.data_ptr(), lum.data_ptr(), nrm.data_ptr(), img.data_ptr(), img8.data_ptr()
    bad_motion = (np.array([1, 0, 0, 0, nan, 0, 0, 0, 1.0]), np.zeros(3))

    def refused(rc, text, status=pm.PM_ERR_INVALID_ARG):
        assert rc == status and lib.pm_last_error(h).decode() == text, (rc, lib.pm_last_error(h).decode(), text)

    # pm_bgr_luma: the images, the output, the shape
    who = "pm_bgr_luma"
    refused(lib.pm_bgr_luma(h, I8, Ip, 0, 0, 0, None), who + ": exactly one of d_bgr8 and d_bgr must be given (both are)")
    refused(lib.pm_bgr_luma(h, None, None, 0, 0, 0, None), who + ": exactly one of d_bgr8 and d_bgr must be given (neither is)")
    refused(lib.pm_bgr_luma(h, I8, None, 0, 0, 0, None), who + ": null d_luma_out")
    refused(lib.pm_bgr_luma(h, None, Ip, 0, cols, 0, bufs["luma"].ptr), who + ": empty image (%dx0)" % cols)
    refused(lib.pm_bgr_luma(h, None, Ip, rows, -3, 0, bufs["luma"].ptr), who + ": empty image (-3x%d)" % rows)
    refused(lib.pm_bgr_luma(h, None, Ip, 70000, 40000, 0, bufs["luma"].ptr),
            who + ": 40000x70000 pixels exceed a 32-bit pixel index or the launch grid", pm.PM_ERR_SIZE)
    assert lib.pm_bgr_luma(None, None, Ip, rows, cols, 0, bufs["luma"].ptr) == pm.PM_ERR_INVALID_ARG

    # pm_align_photo_evaluate: camera, pointers, motion, min_disp, max_diff, huber_levels, shape, outputs
    who = "pm_align_photo_evaluate"
    worst = dict(min_disp=nan, max_diff=-1.0, huber_levels=0.0)

    def evaluate(camera=cam, opt=worst, motion=bad_motion, ptrs=(None, None, None, None), shape=(0, 0), outs=False):
        o = pm.PmAlignPhotoOptions(**opt) if opt is not None else None
        return lib.pm_align_photo_evaluate(h, pm._ref(pm.cloud_camera(camera)), pm._ref(o), pm._ref(pm.as_motion(motion)), *ptrs,
                                           shape[0], shape[1], bufs["cls"].ptr if outs else None, bufs["res"].ptr if outs else None,
                                           bufs["rec"].ptr if outs else None, C.byref(host) if outs else None)

    refused(evaluate(camera=None, opt=None), who + ": null camera")
    refused(evaluate(camera=(nan,) + cam[1:], opt=None), who + ": fx of the camera is not finite")
    refused(evaluate(camera=cam[:4] + (inf,), opt=None), who + ": baseline of the camera is not finite")
    refused(evaluate(camera=(cam[0], 0.0) + cam[2:], opt=None), who + ": fx / fy of the camera must not be 0")
    refused(evaluate(opt=None), who + ": null options")
    for k, name in enumerate(("d_disp_model", "d_luma_model", "d_disp_new", "d_luma_new")):
        refused(evaluate(ptrs=(D, Lp, D, Lp)[:k] + (None,) * (4 - k)), who + ": null " + name)
    all4 = (D, Lp, D, Lp)
    refused(evaluate(ptrs=all4), who + ": R[4] of the motion is not finite")
    refused(evaluate(ptrs=all4, motion=(np.eye(3).ravel(), np.array([0, -inf, 0.0]))), who + ": t[1] of the motion is not finite")
    refused(evaluate(ptrs=all4, motion=None), who + ": min_disp must not be NaN")
    for bad in (-1.0, nan, inf):
        refused(evaluate(ptrs=all4, motion=None, opt=dict(worst, min_disp=0.0, max_diff=bad)), who + ": max_diff must be finite and >= 0")
    for bad in (0.0, -2.0, nan):
        refused(evaluate(ptrs=all4, motion=None, opt=dict(min_disp=0.0, max_diff=1.0, huber_levels=bad)),
                who + ": huber_levels must be > 0 and not NaN")
    good = dict(min_disp=0.0, max_diff=1.0, huber_levels=20.0)
    refused(evaluate(ptrs=all4, motion=None, opt=good), who + ": empty image (0x0)")
    refused(evaluate(ptrs=all4, motion=None, opt=good, shape=(70000, 40000)),
            who + ": 40000x70000 pixels exceed a 32-bit pixel index or the launch grid", pm.PM_ERR_SIZE)
    refused(evaluate(ptrs=all4, motion=None, opt=good, shape=(rows, cols)),
            who + ": no output: d_class_out, d_residual_out, d_sums and sums are all null")
    assert lib.pm_align_photo_evaluate(None, None, None, None, None, None, None, None, 1, 1, None, None, None, None) == pm.PM_ERR_INVALID_ARG

    # pm_align_color_disparity: pm_align_disparity's checks in its order, then the model image, the new images, huber_levels, lambda
    who = "pm_align_color_disparity"
    ok_align = dict(pm.ALIGN_DEFAULTS, min_used=6)
    worst = dict(ok_align, huber_levels=-1.0, lam=-1.0)

    def color(camera=cam, opt=worst, motion=None, dm=D, nm=Np, bm=None, dn=D, b8=None, bf=None, shape=(rows, cols), outs=True):
        o = pm.align_color_options(opt) if opt is not None else None
        return lib.pm_align_color_disparity(h, pm._ref(pm.cloud_camera(camera)), pm._ref(o), pm._ref(pm.as_motion(motion)), dm, nm, bm, dn,
                                            b8, bf, shape[0], shape[1], C.byref(out) if outs else None, C.byref(info) if outs else None)

    refused(color(camera=None), who + ": null camera")
    refused(color(camera=cam[:2] + (nan,) + cam[3:]), who + ": cx of the camera is not finite")
    refused(color(opt=None), who + ": null options")
    refused(color(dm=None), who + ": null d_disp_model")
    refused(color(nm=None), who + ": null d_normals_model")
    refused(color(dn=None), who + ": null d_disp_new")
    refused(color(motion=bad_motion), who + ": R[4] of the guess is not finite")
    refused(color(opt=dict(worst, min_disp=nan)), who + ": min_disp must not be NaN")
    refused(color(opt=dict(worst, max_diff=inf)), who + ": max_diff must be finite and >= 0")
    refused(color(opt=dict(worst, huber_px=0.0)), who + ": huber_px must be > 0 and not NaN")
    refused(color(opt=dict(worst, epsilon=-1.0)), who + ": epsilon must be >= 0 and not NaN")
    refused(color(opt=dict(worst, iterations=51)), who + ": iterations 51 outside 1..50")
    refused(color(opt=dict(worst, min_used=5)), who + ": min_used 5 must be >= 6")
    refused(color(shape=(rows, 0)), who + ": empty image (0x%d)" % rows)
    refused(color(shape=(70000, 40000)), who + ": 40000x70000 pixels exceed a 32-bit pixel index or the launch grid", pm.PM_ERR_SIZE)
    refused(color(outs=False), who + ": no output: out and info are all null")
    refused(color(), who + ": null d_bgr_model")
    refused(color(bm=Ip), who + ": exactly one of d_bgr8_new and d_bgr_new must be given (neither is)")
    refused(color(bm=Ip, b8=I8, bf=Ip), who + ": exactly one of d_bgr8_new and d_bgr_new must be given (both are)")
    refused(color(bm=Ip, b8=I8), who + ": huber_levels must be > 0 and not NaN")
    refused(color(bm=Ip, b8=I8, opt=dict(worst, huber_levels=nan)), who + ": huber_levels must be > 0 and not NaN")
    for bad in (-1.0, nan, inf):
        refused(color(bm=Ip, bf=Ip, opt=dict(worst, huber_levels=20.0, lam=bad)), who + ": lambda must be finite and >= 0")
    assert lib.pm_align_color_disparity(None, None, None, None, None, None, None, None, None, None, 1, 1, None, None) == pm.PM_ERR_INVALID_ARG
    engine.synchronize()
    for buf in bufs.values():
        buf.read(np.uint8, 0)  # the guards and every payload byte still hold the fill
    assert host.n_used == -5 and out.t[0] == 7.0 and info.n_photo_used == -5
    assert (disp.cpu().numpy() == 4.25).all() and (img.cpu().numpy() == 80).all() and (img8.cpu().numpy() == 80).all()
    # and the same arguments made good do run
    assert lib.pm_bgr_luma(h, I8, None, rows, cols, 1, bufs["luma"].ptr) == pm.PM_OK
    assert evaluate(ptrs=all4, motion=None, opt=good, shape=(rows, cols), outs=True) == pm.PM_OK
    flat = lambda v: np.full((rows, cols), v, np.float32)
    used = AP.evaluate(cam, good, IDENT, flat(4.25), flat(80.0), flat(4.25), flat(80.0))["n_used"]
    assert host.n_model == rows * cols and host.n_used == used >= (rows - 2) * (cols - 2)
    assert color(bm=Ip, b8=I8, opt=dict(worst, huber_levels=20.0, lam=0.03)) == pm.PM_OK and info.n_photo_used == used
    engine.synchronize()
    assert np.array_equal(bits(bufs["luma"].read(np.float32)), bits(AP.luma(np.full((rows, cols, 3), 80, np.uint8), True)).ravel())


@gpu
def test_photo_scratch_is_owned_by_the_handle(pm):
    """The second record, the second run of row sums and the two luma planes are ONE further handle-owned allocation, made on
    first use, reused by a call that fits, grown once by a larger map, gone with the handle; the geometric scratch and the bytes
    pm_debug_align_scratch_bytes reports are as they were; one further page-locked record of 240 bytes."""
    import torch
    lib = pm.load()
    live = lambda: (lib.pm_debug_live_device_allocations(), lib.pm_debug_live_device_bytes())
    pinned = lambda: (lib.pm_debug_live_host_buffers(), lib.pm_debug_live_host_bytes())
    before, before_pinned = live(), pinned()
    cam = TA.case_camera((40, 53))
    d = torch.full((40, 53), 4.0, dtype=torch.float32, device="cuda")
    lum = torch.full((40, 53), 9.0, dtype=torch.float32, device="cuda")
    n = torch.zeros((40, 53, 3), dtype=torch.float32, device="cuda")
    n[..., 2] = -1
    img = torch.full((40, 53, 3), 9.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    photo, geo = pm.align_photo_scratch_bytes, pm.align_scratch_bytes
    flat = lambda rows, v: np.full((rows, 53), v, np.float32)
    used = lambda rows: AP.evaluate(cam, AP.photo_options(), IDENT, flat(rows, 4.0), flat(rows, 9.0), flat(rows, 4.0), flat(rows, 9.0))["n_used"]
    assert 18 * 52 <= used(20) <= 20 * 52  # (u, v) is (x, y) up to a rounding, which decides the cell of a row or a column
    assert photo(20, 53) == geo(20) + 8 * 20 * 53 and geo(20) == 256 + 20 * 28 * 8
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        base, base_pinned = live(), pinned()
        run = lambda rows: e.align_photo_evaluate(cam, d.data_ptr(), lum.data_ptr(), d.data_ptr(), lum.data_ptr(), rows, 53, None, None,
                                                  want_sums=True)
        assert run(20).n_used == used(20)
        assert live() == (base[0] + 1, base[1] + photo(20, 53)) and pinned() == (base_pinned[0] + 1, base_pinned[1] + 240)
        assert run(20).n_used == used(20) and run(7).n_used == used(7)
        assert live() == (base[0] + 1, base[1] + photo(20, 53))
        assert run(40).n_used == used(40)
        assert live() == (base[0] + 1, base[1] + photo(40, 53))
        R, t, info = e.align_color_disparity(cam, d.data_ptr(), n.data_ptr(), img.data_ptr(), d.data_ptr(), 40, 53, d_bgr_new=img.data_ptr())
        assert info["n_photo_used"] == used(40) and info["geo"]["valid"] == 0
        assert live() == (base[0] + 2, base[1] + photo(40, 53) + geo(40)) and pinned() == (base_pinned[0] + 2, base_pinned[1] + 480)
        assert e.align_evaluate(cam, d.data_ptr(), n.data_ptr(), d.data_ptr(), 40, 53, None, None, want_sums=True).n_used == 40 * 53
        assert live() == (base[0] + 2, base[1] + photo(40, 53) + geo(40))
    assert live() == before and pinned() == before_pinned


if __name__ == "__main__":
    os.makedirs(os.path.dirname(PROFILE), exist_ok=True)
    open(PROFILE, "w").write(profile_text())
    print(open(PROFILE).read())
