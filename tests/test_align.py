"""Dense frame-to-model alignment (include/pm/imaging.h: pm_align_evaluate, pm_align_step, pm_align_disparity,
pm_motion_compose).

CPU tests pin the definition (tests/align_ref.py) against an ANALYTIC scene -- a ground plane at world Z = 2 m with an off-centre
square pyramid on it, four faces with four distinct normals, whose disparity map at any pose is rendered here by exact ray
intersection, so the maps of different poses are consistent and nothing is resampled -- and run the kernels' own per-thread code
(csrc/pm_align_body.hpp) on the host under ASan / UBSan in the kernels' layout.  GPU tests hold the kernels to the definition with
tolerance 0 -- every operation of the definition is one IEEE rounding, the build uses -ffp-contract=off, the order of the sum is
part of the definition and the kernels keep it -- with guard bands around every buffer."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import align_ref as AR
import normals_fit_ref as NF
import tsdf_ref as TR
from conftest import ROOT
from cpp_build import build_host_kernel
from host_run import assert_program_compares, dump_case
from test_reproject import CAM, FXB, motions

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_align as FA  # noqa: E402  (check_align: the device-against-definition comparison)

gpu = pytest.mark.gpu
rotation = FA.rotation

ROWS, COLS = 48, 80
I3 = np.eye(3).ravel()
IDENT = (I3, np.zeros(3))
PROFILE = os.path.join(ROOT, "profiles", "align_accuracy.txt")

# ---- the analytic scene -------------------------------------------------------------------------------------------------------
Z0 = 2.0                       # the ground plane: world Z = Z0, seen from Z < Z0
APEX = (0.03, -0.02, Z0 - 0.12)  # the pyramid's apex: 12 cm high, off-centre
HALF = 0.15                    # half the width of its square base
# the pyramid is the intersection of five half-spaces n . (X - p) <= 0: four faces through the apex and the base
_SLOPE = (Z0 - APEX[2]) / HALF
PYRAMID = [((sx * _SLOPE, 0.0, -1.0), APEX) for sx in (1.0, -1.0)] + [((0.0, sy * _SLOPE, -1.0), APEX) for sy in (1.0, -1.0)] + \
          [((0.0, 0.0, 1.0), (APEX[0], APEX[1], Z0))]
VOXEL, TRUNC = 0.01, 0.06
GRID = TR.make_grid(52, 34, 40, (-0.255, -0.165, Z0 - 0.3), VOXEL, TRUNC, max_weight=64.0)
RAY = dict(min_range=1.2, max_range=2.4, step=0.5, min_weight=0.0)
CENTRE = np.array([0.0, 0.0, Z0 - 0.06])
FIT = dict(radius=2, max_diff=1.0, min_support=9)   # the normals of a map: tests/normals_fit_ref.py's windowed plane fit
OPT = AR.options(max_diff=1.0, huber_px=0.5, iterations=20, epsilon=1e-10, min_used=200)


def render(pose, rows=ROWS, cols=COLS, cam=CAM):
    """The scene's left disparity map at `pose` (X_cam = R X_world + t) by exact ray intersection, binary64 until the final
    rounding: every pixel's ray against the ground plane and against the pyramid (the ray's interval inside its five
    half-spaces); the nearer wins; +0.0 where the ray meets nothing in front of the camera."""
    fx, fy, cx, cy, baseline = (np.float64(v) for v in cam)
    R = np.asarray(pose[0], np.float64).reshape(3, 3)
    t = np.asarray(pose[1], np.float64)
    c = -(R.T @ t)
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    d_cam = np.stack(np.broadcast_arrays((x - cx) / fx, (y - cy) / fy, np.ones((rows, cols))), -1)
    wd = d_cam @ R  # R^T d per pixel
    with np.errstate(divide="ignore", invalid="ignore"):
        s_plane = (Z0 - c[2]) / wd[..., 2]
        s_plane = np.where(s_plane > 0, s_plane, np.inf)
        lo, hi = np.full((rows, cols), -np.inf), np.full((rows, cols), np.inf)
        for n, p in PYRAMID:
            n, p = np.asarray(n), np.asarray(p)
            den = wd @ n
            s = (n @ (p - c)) / den
            inside = n @ (c - p) <= 0
            lo = np.where(den < 0, np.maximum(lo, s), np.where(den == 0, np.where(inside, lo, np.inf), lo))
            hi = np.where(den > 0, np.minimum(hi, s), hi)
        s_pyr = np.where((lo <= hi) & (lo > 0), lo, np.inf)
        s = np.minimum(s_plane, s_pyr)
        return np.where(np.isfinite(s), (fx * baseline) / s, 0.0).astype(np.float32)


def fit_normals(disp, cam=CAM):
    return NF.disparity_normals(disp, cam, FIT["radius"], FIT["max_diff"], FIT["min_support"])["normals"]


def pose_on_arc(degrees, axis=(0, 1, 0)):
    """The pose of a camera on the circle about CENTRE through the world origin's camera, turned by `degrees` about `axis`."""
    Rwc = rotation(axis, degrees)  # camera to world
    c = CENTRE + Rwc @ np.array([0.0, 0.0, -CENTRE[2]])
    R = Rwc.T
    return R.ravel(), -(R @ c)


def rot_err_deg(Ra, Rb):
    M = np.asarray(Ra).reshape(3, 3) @ np.asarray(Rb).reshape(3, 3).T
    return float(np.degrees(np.arccos(np.clip((np.trace(M) - 1) / 2, -1, 1))))


def motion_error(est, truth):
    """(rotation error in degrees, translation error in metres) of a motion against the true one."""
    return rot_err_deg(est[0], truth[0]), float(np.linalg.norm(np.asarray(est[1]) - np.asarray(truth[1])))


def relative(pose_a, pose_b):
    """The motion from camera a's frame into camera b's: X_b = R_b R_a^T (X_a - t_a) + t_b."""
    Ri, c = TR.FU.inverse_motion(pose_a[0], pose_a[1])
    return AR.compose(pose_b, (Ri, c))


@functools.lru_cache(maxsize=None)
def model_view():
    d = render(IDENT)
    return d, fit_normals(d)


PERTURB_DEG, PERTURB_M = 0.5, 0.004   # the guess: the truth turned by 0.5 degrees about (1, 1, 1) and moved by 4 mm along each axis


def perturbed(truth):
    dR = rotation((1, 1, 1), PERTURB_DEG)
    return (dR @ np.asarray(truth[0]).reshape(3, 3)).ravel(), np.asarray(truth[1]) + PERTURB_M


@functools.lru_cache(maxsize=None)
def aligned_motions():
    """name -> (guess error, reached error, info) for the motions of tests/test_reproject.py on noiseless maps."""
    dm, nm = model_view()
    out = {}
    for name in ("baseline", "advance", "yaw", "roll"):
        truth = motions(CAM, Z0)[name]
        guess = perturbed(truth)
        est, info = AR.align(CAM, OPT, guess, dm, nm, render(truth))
        out[name] = (motion_error(guess, truth), motion_error(est, truth), info)
    return out


ARC_DEG = 5.0
NOISE_PX = 0.3


@functools.lru_cache(maxsize=None)
def sequence():
    """Eight poses on a 5-degree arc, maps with U(-0.3, 0.3) px noise: frame to model (each frame against the tsdf_ref raycast at
    the previous estimated pose, integrated at its estimated pose) and, on the same maps, chained frame-to-frame alignments."""
    rng = np.random.default_rng(12)
    poses = [pose_on_arc(-ARC_DEG / 2 + ARC_DEG * k / 7) for k in range(8)]
    maps = []
    for p in poses:
        d = render(p)
        maps.append(np.where(d > 0, d + rng.uniform(-NOISE_PX, NOISE_PX, d.shape).astype(np.float32), d).astype(np.float32))
    vol = TR.integrate(GRID, TR.clear(GRID), maps[0], CAM, *poses[0])["voxels"]
    pose_m, pose_f = poses[0], poses[0]
    valid_m, valid_f = [], []
    for k in range(1, 8):
        ray = TR.raycast(GRID, vol, CAM, pose_m[0], pose_m[1], ROWS, COLS, **RAY)
        M, info = AR.align(CAM, OPT, IDENT, ray["disp"], ray["normals"], maps[k])
        valid_m.append(info["valid"])
        pose_m = AR.compose(M, pose_m)
        vol = TR.integrate(GRID, vol, maps[k], CAM, *pose_m)["voxels"]
        M, info = AR.align(CAM, OPT, IDENT, maps[k - 1], fit_normals(maps[k - 1]), maps[k])
        valid_f.append(info["valid"])
        pose_f = AR.compose(M, pose_f)
    return dict(model=motion_error(pose_m, poses[-1]), chained=motion_error(pose_f, poses[-1]),
                none=motion_error(poses[0], poses[-1]), valid_m=valid_m, valid_f=valid_f)


def profile_text():
    """The text of profiles/align_accuracy.txt: the reached errors of the definition on the analytic scene."""
    lines = ["# pm_align_disparity's definition (tests/align_ref.py) on the analytic scene of tests/test_align.py: a ground plane at 2 m",
             "# with an off-centre square pyramid (30 cm wide, 12 cm high), %dx%d, noiseless maps, normals from the windowed plane fit" % (COLS, ROWS),
             "# (radius %d).  The guess is the truth turned by %.1f degrees about (1, 1, 1) and moved by %.0f mm along each axis." % (
                 FIT["radius"], PERTURB_DEG, 1e3 * PERTURB_M),
             "# Written by `python tests/test_align.py`; tests/test_align.py asserts twice the reached values below.",
             "# motion     guess: deg  metres    reached: deg  metres    iterations  used  rms_px"]
    for name, (g, r, info) in aligned_motions().items():
        lines.append("motion %-9s guess %.6f %.6f reached %.6f %.6f iterations %d used %d rms_px %.6f" % (
            name, g[0], g[1], r[0], r[1], info["iterations"], info["n_used"], info["rms_px"]))
    s = sequence()
    lines += ["# eight poses on a %.0f-degree arc, maps with U(-%.1f, %.1f) px noise; the pose error of the LAST frame (a record, not a gate):" % (
                  ARC_DEG, NOISE_PX, NOISE_PX),
              "sequence frame-to-model %.6f deg %.6f m" % s["model"],
              "sequence frame-to-frame %.6f deg %.6f m" % s["chained"],
              "sequence no-motion      %.6f deg %.6f m" % s["none"]]
    return "\n".join(lines) + "\n"


def profile_values():
    """name -> (reached deg, reached metres) as profiles/align_accuracy.txt records them."""
    out = {}
    for line in open(PROFILE):
        m = re.match(r"motion (\w+)\s+guess \S+ \S+ reached (\S+) (\S+)", line)
        if m:
            out[m.group(1)] = (float(m.group(2)), float(m.group(3)))
    return out


# ---- 1. the definition ------------------------------------------------------------------------------------------------
def test_the_scene_shows_four_faces_and_the_ground():
    d, n = model_view()
    assert (d > 0).all() and d.max() > FXB / 1.9 and d.min() == np.float32(FXB / Z0)
    ok = np.isfinite(n).all(-1) & (n != 0).any(-1)
    assert ok.mean() > 0.9
    # five clusters of normals: the ground (0, 0, -1) and the four faces, tilted by atan(0.12 / 0.15) about x and y
    tilt = np.array([_SLOPE, 1.0]) / np.hypot(_SLOPE, 1.0)
    for want in ((0, 0, -1), (tilt[0], 0, -tilt[1]), (-tilt[0], 0, -tilt[1]), (0, tilt[0], -tilt[1]), (0, -tilt[0], -tilt[1])):
        assert (np.abs(n[ok] - np.array(want, np.float32)).max(-1) < 0.02).sum() > 60, want


def test_projection_is_the_reprojection_stages():
    """align_ref.project restates reproject_project with its further outputs: it agrees with tsdf_ref.project on what that gives."""
    rng = np.random.default_rng(3)
    X, Y, Z = rng.normal(0, 0.2, 500), rng.normal(0, 0.15, 500), rng.uniform(-1, 4, 500)  # in view, beside it and behind
    R, t = rotation((1, 2, 3), 9.0).ravel(), np.array([0.1, -0.2, 0.3])
    ok, iu, iv, dq, Xn, Yn, Zn = AR.project(CAM, R, t, X, Y, Z, ROWS, COLS)
    ok2, iu2, iv2, Zn2 = TR.project(X, Y, Z, CAM, R, t, ROWS, COLS)
    assert 20 < ok.sum() < 480 and np.array_equal(ok, ok2) and np.array_equal(iu, iu2) and np.array_equal(iv, iv2) and np.array_equal(Zn, Zn2)


def test_a_frame_against_itself_from_the_identity():
    """R = I, t = 0: Xn = (((1 * X) + (0 * Y)) + (0 * Z)) + 0 = X exactly, likewise Yn and Zn, so Q == P bit for bit.
    u = (fx * (X / Z)) + cx with X = (((double)x - cx) * Z) / fx is x up to a few ulps, so rint(u) == x and likewise in y: the
    pixel is associated with itself, d2 == d, P2 == P, every difference Q - P2 is 0 and e, r and every g term are zeros.  H is
    positive definite on this scene, delta = -0 / D = zeros, the Cayley update of the identity by zeros is the identity bit for
    bit (1 +- 0 and 0 + 0 in every entry), max |delta| = 0 < epsilon stops the loop after ONE update."""
    dm, nm = model_view()
    ev = AR.evaluate(CAM, OPT, IDENT, dm, nm, dm)
    assert ev["n_used"] == ev["n_model"] == ev["n_gate"] > 0.9 * ROWS * COLS
    assert (ev["residual"] == 0).all() and (ev["g"] == 0).all() and ev["rr"] == 0 and (ev["H"][[0, 6, 11, 15, 18, 20]] > 0).all()
    (R, t), info = AR.align(CAM, OPT, IDENT, dm, nm, dm)
    assert np.array_equal(R.view(np.uint64), I3.view(np.uint64)) and np.array_equal(t.view(np.uint64), np.zeros(3).view(np.uint64))
    assert info["valid"] == 1 and info["iterations"] == 1 and info["rms_px"] == 0 and info["n_used"] == ev["n_used"]
    assert np.array_equal(info["H"], ev["H"])


def test_a_fronto_parallel_plane_leaves_three_parameters_free():
    """One plane with normal (0, 0, -1): a2 = (P2x * 0) - (P2y * 0) = 0 and m0 = m1 = 0 for every pixel, so the columns of
    omega_z, upsilon_x and upsilon_y are exactly 0, the third pivot is exactly 0, the factorisation fails: valid == 0, no update
    is made and the guess is returned."""
    d = np.full((ROWS, COLS), np.float32(FXB / Z0))
    n = np.zeros((ROWS, COLS, 3), np.float32)
    n[..., 2] = -1
    guess = (rotation((0, 1, 0), 0.2).ravel(), np.array([0.001, 0.0, 0.002]))
    ev = AR.evaluate(CAM, OPT, guess, d, n, d)
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = ev["H"]
    assert ev["n_used"] > 0.9 * ROWS * COLS and (H[0, 0] > 0) and (H[1, 1] > 0) and (H[5, 5] > 0)
    ev0 = AR.evaluate(CAM, OPT, IDENT, d, n, d)
    H0 = np.zeros((6, 6))
    H0[np.triu_indices(6)] = ev0["H"]
    for k in (2, 3, 4):
        assert (H0[k, :] == 0).all() and (H0[:, k] == 0).all(), k
    ok, m, delta = AR.step(ev0["H"], ev0["g"], IDENT)
    assert not ok and (delta == 0).all() and np.array_equal(m[0], I3)
    (R, t), info = AR.align(CAM, OPT, IDENT, d, n, d)
    assert info["valid"] == 0 and info["iterations"] == 0 and np.array_equal(R, I3) and (t == 0).all()
    # under a turned guess the columns are not exactly zero any more, but nothing constrains them: whatever the solve does,
    # an invalid answer is the guess
    (R, t), info = AR.align(CAM, dict(OPT, min_used=ROWS * COLS + 1), guess, d, n, d)
    assert info["valid"] == 0 and np.array_equal(R, guess[0]) and np.array_equal(t, guess[1])


@pytest.mark.parametrize("name", ["baseline", "advance", "yaw", "roll"])
def test_the_motions_of_the_reprojection_tests_are_recovered(name):
    """Noiseless maps, the guess the truth turned by 0.5 degrees about (1, 1, 1) and moved by 4 mm along each axis.  After the
    alignment the rotation error and the translation error are each smaller than the guess's, and within TWICE the value
    profiles/align_accuracy.txt records for this motion.  The factor 2 is slack for the scene generator alone (a different libm
    behind its matrix products and arccos moving a disparity by an ulp): the definition itself is sqrt-free up to rms_px and
    gives the same bits everywhere.  What limits the reached error is the association by nearest pixel."""
    guess, reached, info = aligned_motions()[name]
    recorded = profile_values()[name]
    print(name, "guess", guess, "reached", reached, "recorded", recorded, "iterations", info["iterations"], "used", info["n_used"])
    assert info["valid"] == 1 and info["n_used"] > 0.5 * ROWS * COLS
    assert reached[0] < guess[0] and reached[1] < guess[1]
    assert reached[0] <= 2 * recorded[0] and reached[1] <= 2 * recorded[1]


def test_frame_to_model_tracks_a_noisy_sequence():
    """Eight poses on a 5-degree arc, U(-0.3, 0.3) px noise.  Both chains are valid at every step and frame-to-model's final pose
    error is smaller than that of assuming no motion; how it compares with the frame-to-frame chain is recorded in
    profiles/align_accuracy.txt, not asserted."""
    s = sequence()
    print("frame to model", s["model"], "frame to frame", s["chained"], "no motion", s["none"])
    assert all(s["valid_m"]) and all(s["valid_f"])
    assert s["model"][0] < s["none"][0] and s["model"][1] < s["none"][1]


def test_the_profile_is_what_the_definition_gives_within_its_slack():
    values = profile_values()
    assert set(values) == {"baseline", "advance", "yaw", "roll"}
    text = open(PROFILE).read()
    assert "sequence frame-to-model" in text and "sequence frame-to-frame" in text


# ---- 2. every class and every branch ------------------------------------------------------------------------------------------
def class_cases():
    """(name, motion, Dm, Nm, Dn, options) on a 6x9 map of one plane; each produces the class(es) its name says."""
    rows, cols = 6, 9
    cam = (30.0, 28.0, 4.2, 2.6, 0.1)
    d0 = np.float32(cam[0] * cam[4] / 1.5)
    Dm = np.full((rows, cols), d0, np.float32)
    Nm = np.zeros((rows, cols, 3), np.float32)
    Nm[..., 2] = -1
    Nm[..., 0] = 0.25
    opt = AR.options(max_diff=0.6, huber_px=0.25, min_used=6)
    cases = {}
    cases["used, both Huber branches"] = (IDENT, Dm, Nm, Dm + np.where(np.arange(cols) % 2, np.float32(0.5), np.float32(0.1))[None, :], opt)
    cases["behind the camera"] = ((I3, np.array([0.0, 0.0, -10.0])), Dm, Nm, Dm, opt)
    cases["outside the image"] = ((I3, np.array([100.0, 0.0, 0.0])), Dm, Nm, Dm, opt)
    Dn = Dm.copy()
    Dn[0, :4] = (0.0, -0.0, np.nan, -3.0)
    Dn[1, 0] = d0 + 5  # an occluder in front of the model
    Dn[1, 1] = d0 - 1  # the model in front of what the frame sees
    cases["unmeasured and gated"] = (IDENT, Dm, Nm, Dn, opt)
    Dm2, Nm2 = Dm.copy(), Nm.copy()
    Dm2[2, :3] = (0.0, np.nan, -1.0)
    Nm2[3, 0] = 0
    Nm2[3, 1, 1] = np.nan
    Nm2[3, 2, 0] = np.inf
    cases["no model"] = (IDENT, Dm2, Nm2, Dm, opt)
    cases["min_disp"] = (IDENT, Dm, Nm, Dm, dict(opt, min_disp=float(d0) + 1))
    return cam, cases


def test_every_class_is_produced_and_every_branch_is_reached():
    cam, cases = class_cases()
    seen, weights = set(), set()
    for name, (motion, Dm, Nm, Dn, opt) in cases.items():
        ev = AR.evaluate(cam, opt, motion, Dm, Nm, Dn)
        c = ev["cls"]
        seen |= set(int(v) for v in np.unique(c))
        assert ev["n_model"] == (c != 0).sum() and ev["n_gate"] == (c >= 3).sum() and ev["n_used"] == (c == 4).sum()
        assert (ev["residual"][c != AR.USED] == 0).all() and not np.signbit(ev["residual"][c != AR.USED]).any()
        if name == "used, both Huber branches":
            assert (c == AR.USED).all()
            r = np.abs(ev["residual"].astype(np.float64))
            weights |= {"one" if v <= opt["huber_px"] else "less" for v in r.ravel()}
            assert (r > 0).all()
        if name in ("behind the camera", "outside the image"):
            assert (c == AR.OUTSIDE).all() and ev["n_model"] == c.size and ev["n_gate"] == 0
        if name == "unmeasured and gated":
            assert (c[0, :4] == AR.UNMEASURED).all() and (c[1, :2] == AR.GATED).all() and (c[2:] == AR.USED).all()
        if name == "no model":
            assert (c[2, :3] == AR.NO_MODEL).all() and (c[3, :3] == AR.NO_MODEL).all() and (c[4:] == AR.USED).all()
        if name == "min_disp":
            assert (c == AR.NO_MODEL).all() and (ev["H"] == 0).all()
    assert seen == {0, 1, 2, 3, 4} and weights == {"one", "less"}


def test_the_order_of_the_sum_is_the_definitions():
    """ordered_sum against a scalar restatement: lanes over chunks, the tree, the rows; and it is not numpy's own sum."""
    rng = np.random.default_rng(5)
    for rows, cols in ((1, 1), (1, 65), (3, 130), (5, 64)):
        T = rng.normal(0, 1, (rows, cols, AR.TERMS)) * 10.0 ** rng.integers(-8, 8, (rows, cols, 1))
        total, row_sums = AR.ordered_sum(T)
        for e in (0, 13, 27):
            want = 0.0
            for y in range(rows):
                s = [0.0] * 64
                for x in range(cols):
                    s[x % 64] = s[x % 64] + T[y, x, e]
                while len(s) > 1:
                    s = [s[2 * i] + s[2 * i + 1] for i in range(len(s) // 2)]
                assert s[0] == row_sums[y, e]
                want = want + s[0]
            assert want == total[e]
    assert (AR.ordered_sum(T)[0] != T.sum((0, 1))).any()


def dpp_tree(v):
    """numpy restatement of the kernel's wave_sum_f64: the DPP sequence quad_perm [1,0,3,2], quad_perm [2,3,0,1],
    row_half_mirror, row_mirror, row_bcast15 (rows 1 and 3), row_bcast31 (rows 2 and 3) -> what lane 63 holds."""
    v = np.asarray(v, np.float64).copy()
    lane = np.arange(64)
    v = v + v[lane ^ 1]
    v = v + v[lane ^ 2]
    v = v + v[(lane & ~7) | (7 - (lane & 7))]
    v = v + v[(lane & ~15) | (15 - (lane & 15))]
    row = lane // 16
    v = v + np.where((row == 1) | (row == 3), v[np.maximum(row * 16 - 1, 0)], 0.0)
    v = v + np.where(row >= 2, v[31], 0.0)
    return v[63]


def test_the_dpp_sequence_is_the_balanced_tree_bit_for_bit():
    rng = np.random.default_rng(6)
    for k in range(200):
        v = rng.normal(0, 1, 64) * 10.0 ** rng.integers(-12, 12, 64)
        if k % 5 == 0:
            v[rng.random(64) < 0.5] = 0.0
        assert dpp_tree(v) == AR.tree(v) and np.float64(dpp_tree(v)).view(np.uint64) == np.float64(AR.tree(v)).view(np.uint64)
    assert any(AR.tree(v) != np.cumsum(v)[-1] for v in rng.normal(0, 1, (20, 64)))  # and it is not the sum in lane order


def seeded_sums(rng, singular=False):
    A = rng.normal(0, 1, (40, 6))
    if singular:
        A[:, 2] = 0.0  # the third pivot is exactly 0
    H = A.T @ A
    return [H[i, j] for i in range(6) for j in range(i, 6)], rng.normal(0, 0.01, 6)


def test_step_and_compose_equal_the_reference_bit_for_bit(pm):
    rng = np.random.default_rng(7)
    failures = 0
    for k in range(40):
        H21, g = seeded_sums(rng, singular=k % 8 == 3)
        motion = None if k % 5 == 0 else (rotation(rng.normal(size=3), rng.uniform(-20, 20)).ravel(), rng.normal(0, 1, 3))
        ok, R, t, delta = pm.align_step(pm.align_sums(H21, g), motion)
        wok, (wR, wt), wdelta = AR.step(H21, g, motion or IDENT)
        assert ok == wok
        for got, want in ((R, wR), (t, wt), (delta, wdelta)):
            assert np.array_equal(got.view(np.uint64), np.asarray(want, np.float64).view(np.uint64)), (k, got, want)
        failures += not ok
        if not ok:
            assert (delta == 0).all() and np.array_equal(R, (motion or IDENT)[0])
        b = (rotation(rng.normal(size=3), rng.uniform(-90, 90)).ravel(), rng.normal(0, 1, 3))
        a = (R, t)
        for got, want in zip(pm.motion_compose(a, b), AR.compose(a, b)):
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert failures == 5
    lib = pm.load()
    s, m = pm.align_sums(*seeded_sums(rng)), pm.PmMotion()
    assert lib.pm_align_step(None, None, C.byref(m), None, None) == pm.PM_ERR_INVALID_ARG
    assert lib.pm_align_step(C.byref(s), None, None, None, None) == pm.PM_ERR_INVALID_ARG
    assert lib.pm_align_step(C.byref(s), None, C.byref(m), None, None) == pm.PM_OK
    for args in ((None, C.byref(m), C.byref(m)), (C.byref(m), None, C.byref(m)), (C.byref(m), C.byref(m), None)):
        assert lib.pm_motion_compose(*args) == pm.PM_ERR_INVALID_ARG
    # a pose from a render: compose(M, pose_ref) maps the world into the new camera
    pose_ref, M = pose_on_arc(3.0), (rotation((0, 1, 0), 1.0).ravel(), np.array([0.01, 0.0, 0.0]))
    X = np.array([0.1, -0.2, 2.0])
    R, t = pm.motion_compose(M, pose_ref)
    direct = M[0].reshape(3, 3) @ (pose_ref[0].reshape(3, 3) @ X + pose_ref[1]) + M[1]
    assert np.abs(R.reshape(3, 3) @ X + t - direct).max() < 1e-14


# ---- 3. the kernels' code on the host ----------------------------------------------------------------------------------------------
SHAPES = {"1x1": (1, 1), "1x63": (1, 63), "1x64": (1, 64), "1x65": (1, 65), "3x130": (3, 130), "5x64": (5, 64), "37x53": (37, 53)}
MOTIONS = ("identity", "yaw", "roll", "behind", "beside")
KINDS = ("noise", "constants", "specials")


def case_camera(shape):
    rows, cols = shape
    f = 1.3 * max(cols, 16)
    return (f, 0.95 * f, cols / 2 - 0.3, rows / 2 + 0.2, 0.1)


def case_motion(name, depth):
    return {"identity": IDENT, "yaw": (rotation((0, 1, 0), 2.0).ravel(), np.zeros(3)), "roll": (rotation((0, 0, 1), 7.0).ravel(), np.zeros(3)),
            "behind": (I3, np.array([0.0, 0.0, -3.0 * depth])), "beside": (I3, np.array([100.0 * depth, 0.0, 0.0]))}[name]


@functools.lru_cache(maxsize=None)
def align_case(shape_name, motion_name, kind):
    """(camera, options, motion, Dm, Nm, Dn, the definition's evaluation) of a fixed case."""
    if shape_name == "scene":
        dm, nm = model_view()
        truth = motions(CAM, Z0)["yaw"] if motion_name == "identity" else case_motion(motion_name, Z0)
        dn = render(truth)
        if kind == "specials":
            dn = dn.copy()
            dn[::5, ::7] = FA.SPECIALS[np.arange(dn[::5, ::7].size) % len(FA.SPECIALS)].reshape(dn[::5, ::7].shape)
        elif kind == "noise":
            dn = (dn + np.random.default_rng(2).uniform(-0.3, 0.3, dn.shape)).astype(np.float32)
        cam, opt, motion = CAM, OPT, case_motion(motion_name, Z0)
        return cam, opt, motion, dm, nm, dn, AR.evaluate(cam, opt, motion, dm, nm, dn)
    rows, cols = shape = SHAPES[shape_name]
    cam = case_camera(shape)
    depth = 1.5
    mid = cam[0] * cam[4] / depth
    seed = sum(map(ord, shape_name + motion_name + kind))
    rng = np.random.default_rng(seed)
    if kind == "constants":
        dm = np.full(shape, mid, np.float32)
        dn = np.full(shape, mid * 1.01, np.float32)
        nm = np.broadcast_to(np.array([0.3, -0.2, -0.93], np.float32), shape + (3,)).copy()
    else:
        special = 0.15 if kind == "specials" else 0.0
        dm = FA.random_disp(rng, rows, cols, valid=1.0 if kind == "noise" else 0.8, special=special, lo=0.95 * mid, hi=1.05 * mid)
        dn = FA.random_disp(rng, rows, cols, valid=1.0 if kind == "noise" else 0.8, special=special, lo=0.95 * mid, hi=1.05 * mid)
        nm = FA.random_normals(rng, rows, cols, special=special / 2)
    opt = AR.options(max_diff=0.06 * mid, huber_px=0.02 * mid, min_used=6)
    motion = case_motion(motion_name, depth)
    return cam, opt, motion, dm, nm, dn, AR.evaluate(cam, opt, motion, dm, nm, dn)


def test_conditions_the_cases_use_gate_and_drop_pixels():
    """The fixed cases are not empty: pixels are used under the identity, the yaw and the roll, in every kind of map, both Huber
    branches and every class occur, and the motions behind and beside the scene use nothing."""
    classes = set()
    for shape in ("37x53", "3x130", "scene"):
        for motion in MOTIONS:
            for kind in KINDS:
                *_, ev = align_case(shape, motion, kind)
                classes |= set(int(v) for v in np.unique(ev["cls"]))
                if motion in ("behind", "beside"):  # (a subnormal disparity is a point 1e46 m away: it stays in front)
                    assert (ev["n_used"] == 0 or kind == "specials") and ev["n_model"] > 0, (shape, motion, kind)
                else:
                    assert ev["n_used"] > 5 and ev["rr"] > 0, (shape, motion, kind, ev["n_used"])
    assert classes == {0, 1, 2, 3, 4}
    _, opt, _, _, _, _, ev = align_case("37x53", "yaw", "noise")
    r = np.abs(ev["residual"][ev["cls"] == AR.USED])
    assert (r <= opt["huber_px"]).any() and (r > opt["huber_px"]).any()


@pytest.fixture(scope="module")
def host_align_exe(tmp_path_factory):
    """tests/cpp/align_host_main.cpp: csrc/pm_align_body.hpp compiled for the host alone, with the sanitizers."""
    return build_host_kernel(tmp_path_factory.mktemp("alignhost") / "align_host_main", "align_host_main.cpp")


def _dump_case(path, cam, opt, motion, dm, nm, dn, ev):
    dump_case(path, [*cam, *dm.shape, opt["min_disp"], opt["max_diff"], opt["huber_px"], *np.asarray(motion[0]).ravel(), *motion[1]],
              disp_model=dm, normals_model=nm, disp_new=dn, want_record=AR.record(ev), want_class=ev["cls"], want_residual=ev["residual"])


def test_kernel_code_on_the_host_equals_the_definition(host_align_exe, tmp_path):
    """pm_align_body.hpp composed serially in the kernels' layout -- lane sums, tree, rows -- over 1x1, 1x65, 5x64, 3x130 and
    37x53, blocks and threads forwards and backwards, each optional plane alone and neither: the 240-byte record, the classes
    and the residuals equal the .npy dumps of the definition byte for byte, and AddressSanitizer / UBSan see every access into
    buffers of exactly the size the stage may touch."""
    used, k = 0, 0
    for shape in ("1x1", "1x65", "5x64", "3x130", "37x53"):
        for motion in MOTIONS:
            kind = KINDS[k % 3]
            cam, opt, m, dm, nm, dn, ev = align_case(shape, motion, kind)
            d = str(tmp_path / ("case%d" % k))
            _dump_case(d, cam, opt, m, dm, nm, dn, ev)
            r = subprocess.run([host_align_exe, d], capture_output=True, text=True)
            assert r.returncode == 0, (shape, motion, kind, r.stderr[-3000:])
            used += ev["n_used"]
            k += 1
    assert used > 3000
    cam, opt, m, dm, nm, dn, ev = align_case("37x53", "roll", "noise")
    d = str(tmp_path / "flip")
    _dump_case(d, cam, opt, m, dm, nm, dn, ev)
    assert ev["n_used"] > 500
    assert_program_compares(host_align_exe, d, [("want_record", np.uint8, "the record differs"), ("want_class", np.uint8, "the classes differ"),
                                                ("want_residual", np.uint32, "the residuals differ")])


def test_headers_declare_and_the_library_exports_the_align_functions(pm):
    text = open(os.path.join(ROOT, "include", "pm", "imaging.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = pm.load()
    for name in ("pm_align_evaluate", "pm_align_disparity"):
        assert re.search(r"\bint\s+%s\s*\(\s*pm_handle\s*\*" % name, text), name
    assert re.search(r"\bint\s+pm_align_step\s*\(\s*const\s+pm_align_sums\s*\*", text)
    assert re.search(r"\bint\s+pm_motion_compose\s*\(\s*const\s+pm_motion\s*\*", text)
    for name in ("pm_align_evaluate", "pm_align_step", "pm_align_disparity", "pm_motion_compose", "pm_debug_align_constants",
                 "pm_debug_align_scratch_bytes"):
        assert name in pm.EXPORTS and hasattr(lib, name), name
    for name in ("pm_align_options", "pm_align_sums", "pm_align_info"):
        assert "typedef struct " + name in text, name
    assert text.index("pm_tsdf_mesh") < text.index("pm_align_evaluate") < text.index("pm_device_malloc")
    assert "#define PM_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "pm", "patchmatch.h")).read() and pm.PM_ABI_VERSION == 6
    assert (C.sizeof(pm.PmAlignOptions), C.sizeof(pm.PmAlignSums), C.sizeof(pm.PmAlignInfo)) == (40, 240, 200)
    assert pm.align_constants() == (64, 4) and pm.align_scratch_bytes(720) == 256 + 720 * 28 * 8 and pm.align_scratch_bytes(0) == 0
    csrc = os.path.join(ROOT, "ocean-perception_amd", "csrc")
    assert '#include "pm_align.hpp"' in open(os.path.join(csrc, "pm_stages.hip")).read()  # the kernels live in that unit alone
    assert "pm_align.hpp" in open(os.path.join(csrc, "pm_handle.hpp")).read()
    for f in os.listdir(csrc):
        if f.endswith(".hip") and f != "pm_stages.hip":
            assert "pm_align" not in open(os.path.join(csrc, f)).read(), f
    host = os.path.join(ROOT, "ocean-perception_amd", "host")
    for f in ("motion.cpp", "align.cpp"):  # the solve and the update are stated once
        src = open(os.path.join(host, f)).read()
        assert '#include "motion_solve.hpp"' in src and "ldlt_solve(const" not in src, f


# ---- 4. device parity ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        yield e


def _check(torch, engine, shape, motion, kind, outputs=FA.OUTPUTS, offset_floats=0):
    cam, opt, m, dm, nm, dn, ev = align_case(shape, motion, kind)
    return FA.check_align(torch, engine, cam, opt, m, dm, nm, dn, outputs, offset_floats, want=ev)


@gpu
@pytest.mark.parametrize("shape", list(SHAPES) + ["scene"])
def test_align_evaluate_equals_the_definition(pm, engine, shape):
    """One pixel; the chunk edge (63, 64 and 65 pixels in a row); three chunks per lane sum and three rows; rows beyond one block;
    a map that is no multiple of anything; the 48x80 scene -- each under the identity, a yaw, a roll and motions that put the
    model behind and beside the camera, with maps from noise, constants and every special value, the inputs 4, 8 and 12 bytes
    past a 16-byte boundary in turn: the record on the device and on the host, the classes and the residuals at tolerance 0."""
    import torch
    k = 0
    for motion in MOTIONS:
        for kind in KINDS:
            _check(torch, engine, shape, motion, kind, offset_floats=k % 4)
            k += 1


@gpu
def test_each_output_alone_and_absent_and_two_runs_agree(pm, engine):
    import torch
    four = FA.OUTPUTS
    for outputs in [tuple(k for k in four if k != drop) for drop in four] + [(k,) for k in four]:
        _check(torch, engine, "37x53", "roll", "specials", outputs=outputs)
        _check(torch, engine, "3x130", "yaw", "noise", outputs=outputs, offset_floats=1)
    # two equal runs give equal bytes (and both the definition's: checked above); here on the device record directly
    cam, opt, m, dm, nm, dn, ev = align_case("scene", "yaw", "noise")
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (dm, nm, dn)]
    recs = [FA.Guarded(torch, 240) for _ in range(2)]
    torch.cuda.synchronize()
    for rec in recs:
        engine.align_evaluate(cam, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), ROWS, COLS, m, opt, d_sums=rec.ptr)
    engine.synchronize()
    a, b = (rec.read(np.uint8) for rec in recs)
    assert np.array_equal(a, b) and np.array_equal(a, AR.record(ev))


@gpu
@pytest.mark.parametrize("name", ["identity", "yaw", "plane"])
def test_align_disparity_equals_the_definitions_loop(pm, engine, name):
    """pm_align_disparity on the scene equals align_ref.align bit for bit -- the motion, the info and H: a frame against itself
    (one update, the identity), the 2-degree yaw from a perturbed guess, and the fronto-parallel plane whose factorisation fails
    (valid == 0, the guess returned)."""
    import torch
    dm, nm = model_view()
    if name == "identity":
        want = FA.check_align_disparity(torch, engine, CAM, OPT, None, dm, nm, dm)
        assert want[1]["iterations"] == 1 and want[1]["valid"] == 1
    elif name == "yaw":
        truth = motions(CAM, Z0)["yaw"]
        want = FA.check_align_disparity(torch, engine, CAM, OPT, perturbed(truth), dm, nm, render(truth))
        assert want[1]["valid"] == 1 and want[1]["iterations"] > 1
    else:
        d = np.full((ROWS, COLS), np.float32(FXB / Z0))
        n = np.zeros((ROWS, COLS, 3), np.float32)
        n[..., 2] = -1
        want = FA.check_align_disparity(torch, engine, CAM, OPT, None, d, n, d)
        assert want[1]["valid"] == 0 and want[1]["iterations"] == 0


@gpu
def test_align_directly_behind_a_raycast_on_the_handles_stream(pm, engine):
    """clear, integrate, raycast and evaluate on the handle's stream with nothing copied and nothing synchronised in between: the
    record equals the definition on the definition's own raycast."""
    import torch
    truth = motions(CAM, Z0)["yaw"]
    d0, d1 = render(IDENT), render(truth)
    vol = FA.Guarded(torch, 8 * GRID["nx"] * GRID["ny"] * GRID["nz"])
    t0, t1 = torch.from_numpy(d0).cuda(), torch.from_numpy(d1).cuda()
    out, nrm, rec = FA.Guarded(torch, 4 * ROWS * COLS), FA.Guarded(torch, 12 * ROWS * COLS), FA.Guarded(torch, 240)
    torch.cuda.synchronize()
    engine.tsdf_clear(GRID, vol.ptr)
    engine.tsdf_integrate(CAM, GRID, IDENT, t0.data_ptr(), ROWS, COLS, vol.ptr)
    engine.tsdf_raycast(CAM, GRID, IDENT, vol.ptr, ROWS, COLS, d_disp_out=out.ptr, d_normals_out=nrm.ptr, **RAY)
    engine.align_evaluate(CAM, out.ptr, nrm.ptr, t1.data_ptr(), ROWS, COLS, truth, OPT, d_sums=rec.ptr)
    engine.synchronize()
    ray = TR.raycast(GRID, TR.integrate(GRID, TR.clear(GRID), d0, CAM, *IDENT)["voxels"], CAM, *IDENT, ROWS, COLS, **RAY)
    ev = AR.evaluate(CAM, OPT, truth, ray["disp"], ray["normals"], d1)
    assert ev["n_used"] > 0.5 * ROWS * COLS
    assert np.array_equal(rec.read(np.uint8), AR.record(ev))


@gpu
@pytest.mark.parametrize("mode", ["scalar", "planes"])
def test_align_directly_behind_a_match_on_the_handles_stream(pm, synth, mode):
    """A Match() of a synthetic pair into a device buffer, then its normals by the plane fit and an evaluation of the map against
    itself under a small motion, all on the handle's stream with nothing synchronised in between: the record equals the definition
    on the downloaded map and normals."""
    import torch
    rows, cols = 96, 128
    cam = (100.0, 100.0, 64.0, 48.0, 0.02)
    kw = dict(mode=pm.PM_MODE_PLANES) if mode == "planes" else {}
    p = synth.make_pair(5, rows=rows, cols=cols, n_points=40, dilate_factor=2)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    L, R, SL, SR = (up(p[k]) for k in ("left", "right", "seed_l", "seed_r"))
    D = torch.zeros((2, rows, cols), dtype=torch.float32, device="cuda")
    N = torch.zeros((rows, cols, 3), dtype=torch.float32, device="cuda")
    rec = FA.Guarded(torch, 240)
    motion = (rotation((0, 1, 0), 0.3).ravel(), np.array([0.001, 0.0, 0.0]))
    opt = AR.options(max_diff=2.0, huber_px=0.5, min_used=6)
    torch.cuda.synchronize()
    with pm.Engine(pm.default_params(0, patch=5, patchmatch_iters=2, max_disp=32, **kw), max_rows=rows, max_cols=cols) as e:
        e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), D[0].data_ptr(), D[1].data_ptr())
        fit = pm.PmNormalsFit(2, 1.0, 9)
        e._check(e.lib.pm_disparity_normals(e.h, pm._ref(pm.cloud_camera(cam)), C.byref(fit), D[0].data_ptr(), rows, cols,
                                            N.data_ptr(), None, None), "pm_disparity_normals")
        e.align_evaluate(cam, D[0].data_ptr(), N.data_ptr(), D[0].data_ptr(), rows, cols, motion, opt, d_sums=rec.ptr)
        e.synchronize()
    disp, normals = D[0].cpu().numpy(), N.cpu().numpy()
    ev = AR.evaluate(cam, opt, motion, disp, normals, disp)
    print(mode, "model", ev["n_model"], "gate", ev["n_gate"], "used", ev["n_used"])
    assert ev["n_used"] > 500
    assert np.array_equal(rec.read(np.uint8), AR.record(ev))


@gpu
def test_invalid_arguments_are_named_and_nothing_is_enqueued(pm, engine):
    """PM_ERR_INVALID_ARG / PM_ERR_SIZE with pm_last_error naming the argument; the outputs keep their guard patterns and their
    payloads, the host outputs their values."""
    import torch
    rows, cols = 16, 24
    lib, h = engine.lib, engine.h
    cam = (40.0, 40.0, 12.0, 8.0, 0.1)
    disp = torch.full((rows, cols), 4.25, dtype=torch.float32, device="cuda")
    nrm = torch.zeros((rows, cols, 3), dtype=torch.float32, device="cuda")
    nrm[..., 2] = -1
    nrm[..., 0] = torch.linspace(-0.5, 0.5, cols, device="cuda")[None, :]
    nrm[..., 1] = torch.linspace(-0.5, 0.5, rows, device="cuda")[:, None]
    bufs = {k: FA.Guarded(torch, n) for k, n in (("cls", rows * cols), ("res", 4 * rows * cols), ("rec", 240))}
    host = pm.PmAlignSums()
    host.n_used = -5
    out, info = pm.PmMotion(), pm.PmAlignInfo()
    out.t[0], info.valid = 7.0, -5
    UNSET = object()
    pick = lambda v, default: default if v is UNSET else v
    good = dict(pm.ALIGN_DEFAULTS, min_used=6)

    def evaluate(camera=cam, opt=UNSET, motion=IDENT, dm=UNSET, nm=UNSET, dn=UNSET, shape=(rows, cols), outs=True):
        o = pm.PmAlignOptions(**pick(opt, good)) if opt is not None else None
        return lib.pm_align_evaluate(h, pm._ref(pm.cloud_camera(camera)), pm._ref(o), pm._ref(pm.as_motion(motion)),
                                     pick(dm, disp.data_ptr()), pick(nm, nrm.data_ptr()), pick(dn, disp.data_ptr()), shape[0], shape[1],
                                     bufs["cls"].ptr if outs else None, bufs["res"].ptr if outs else None,
                                     bufs["rec"].ptr if outs else None, C.byref(host) if outs else None)

    def disparity(camera=cam, opt=UNSET, motion=IDENT, dm=UNSET, nm=UNSET, dn=UNSET, shape=(rows, cols), outs=True):
        o = pm.PmAlignOptions(**pick(opt, good)) if opt is not None else None
        return lib.pm_align_disparity(h, pm._ref(pm.cloud_camera(camera)), pm._ref(o), pm._ref(pm.as_motion(motion)),
                                      pick(dm, disp.data_ptr()), pick(nm, nrm.data_ptr()), pick(dn, disp.data_ptr()), shape[0], shape[1],
                                      C.byref(out) if outs else None, C.byref(info) if outs else None)

    def refused(rc, word, who, status=pm.PM_ERR_INVALID_ARG):
        text = lib.pm_last_error(h).decode()
        assert rc == status and word in text and who in text, (rc, word, text)

    nan, inf = float("nan"), float("inf")
    for call, who, whose in ((evaluate, "pm_align_evaluate", "the motion"), (disparity, "pm_align_disparity", "the guess")):
        refused(call(camera=None), "camera", who)
        refused(call(opt=None), "options", who)
        refused(call(dm=None), "d_disp_model", who)
        refused(call(nm=None), "d_normals_model", who)
        refused(call(dn=None), "d_disp_new", who)
        for i, name in enumerate(("fx", "fy", "cx", "cy", "baseline")):
            for bad in (nan, inf, -inf):
                refused(call(camera=cam[:i] + (bad,) + cam[i + 1:]), name, who)
        refused(call(camera=(0.0,) + cam[1:]), "fx", who)
        refused(call(camera=(cam[0], 0.0) + cam[2:]), "fy", who)
        for i in range(12):
            for bad in (nan, inf, -inf):
                R, t = np.eye(3).ravel(), np.zeros(3)
                (R if i < 9 else t)[i if i < 9 else i - 9] = bad
                refused(call(motion=(R, t)), ("R[%d]" % i if i < 9 else "t[%d]" % (i - 9)) + " of " + whose, who)
        refused(call(opt=dict(good, min_disp=nan)), "min_disp", who)
        for bad in (nan, inf, -0.5):
            refused(call(opt=dict(good, max_diff=bad)), "max_diff", who)
        for bad in (nan, 0.0, -1.0):
            refused(call(opt=dict(good, huber_px=bad)), "huber_px", who)
        for bad in (0, -1, 51):
            refused(call(opt=dict(good, iterations=bad)), "iterations", who)
        for bad in (nan, -1e-9):
            refused(call(opt=dict(good, epsilon=bad)), "epsilon", who)
        for bad in (5, 0, -3):
            refused(call(opt=dict(good, min_used=bad)), "min_used", who)
        for shape in ((0, cols), (rows, 0), (rows, -3)):
            refused(call(shape=shape), "empty", who)
        refused(call(shape=(70000, 40000)), "exceed", who, pm.PM_ERR_SIZE)
        refused(call(outs=False), "no output", who)
    assert lib.pm_align_evaluate(None, None, None, None, None, None, None, 1, 1, None, None, None, None) == pm.PM_ERR_INVALID_ARG
    engine.synchronize()
    for buf in bufs.values():
        buf.read(np.uint8, 0)  # the guards and every payload byte still hold the fill
    assert host.n_used == -5 and out.t[0] == 7.0 and info.valid == -5 and (disp.cpu().numpy() == 4.25).all()
    # and the same arguments made good do run
    assert evaluate() == pm.PM_OK and host.n_used == rows * cols == host.n_model
    assert disparity() == pm.PM_OK and info.n_used == rows * cols and info.valid in (0, 1)


@gpu
def test_align_scratch_is_owned_by_the_handle(pm):
    """The row sums and the record are ONE handle-owned allocation through csrc/pm_devbuf.hpp, made on first use, reused by a call
    that fits, grown once by a taller map, gone with the handle; the page-locked record is one host buffer of 240 bytes."""
    import torch
    lib = pm.load()
    live = lambda: (lib.pm_debug_live_device_allocations(), lib.pm_debug_live_device_bytes())
    pinned = lambda: (lib.pm_debug_live_host_buffers(), lib.pm_debug_live_host_bytes())
    before, before_pinned = live(), pinned()
    cam = case_camera((40, 53))
    d = torch.full((40, 53), 4.0, dtype=torch.float32, device="cuda")
    n = torch.zeros((40, 53, 3), dtype=torch.float32, device="cuda")
    n[..., 2] = -1
    torch.cuda.synchronize()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        base, base_pinned = live(), pinned()
        run = lambda rows: e.align_evaluate(cam, d.data_ptr(), n.data_ptr(), d.data_ptr(), rows, 53, None, None, want_sums=True)
        assert run(20).n_used == 20 * 53
        assert live() == (base[0] + 1, base[1] + pm.align_scratch_bytes(20)) and pinned() == (base_pinned[0] + 1, base_pinned[1] + 240)
        assert run(20).n_used == 20 * 53 and run(7).n_used == 7 * 53
        assert live() == (base[0] + 1, base[1] + pm.align_scratch_bytes(20))
        assert run(40).n_used == 40 * 53
        assert live() == (base[0] + 1, base[1] + pm.align_scratch_bytes(40))
        R, t, info = e.align_disparity(cam, d.data_ptr(), n.data_ptr(), d.data_ptr(), 40, 53)
        assert info["valid"] == 0 and live() == (base[0] + 1, base[1] + pm.align_scratch_bytes(40)) and pinned()[0] == base_pinned[0] + 1
    assert live() == before and pinned() == before_pinned


@gpu
def test_fuzz_align_one_short_seeded_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_align.py"), "--cases", "16", "--seed", "4"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


if __name__ == "__main__":
    os.makedirs(os.path.dirname(PROFILE), exist_ok=True)
    open(PROFILE, "w").write(profile_text())
    print(open(PROFILE).read())
