"""Differential fuzz of pm_track_features and pm_estimate_motion (through the C ABI) against the CPU definition
(tests/motion_ref.py).  Random shapes <= 96x160; old and new images that are noise, binary 0/255 noise, periodic textures,
ramps, or a rendered scene and its shifted copy; disparity maps with every special value (0, -0.0, negatives, NaN, +inf,
subnormals); guesses from the identity to one that throws every prediction out of the image or behind the camera; every option
over its whole range; capacities from 0 past the count.  Tolerance 0: every record, the count and the solved motion bit-exact,
guard bands around the records intact, or it prints the case and exits 1.  check_motion / check_estimate are what
tests/test_motion.py runs its fixed cases through; scene() renders the analytic two-surface scene of its accuracy tests.

    python tools/fuzz_motion.py [--cases 40] [--seed 1] [--max-rows 96] [--max-cols 160]
    python tools/fuzz_motion.py --accuracy      (no GPU: writes profiles/motion_accuracy.txt from the definition alone)
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import motion_ref as MR
from fuzz_cloud import Guarded, SPECIALS, bits, random_disp  # noqa: F401  (re-exported to the tests)
from fuzz_reproject import IDENTITY, random_motion, rotation  # noqa: F401


# ---- an analytic scene: a textured slanted plane with a nearer fronto-parallel patch in front of it -------------------------------
def _value_noise(table, u, v):
    """Bilinear interpolation of a periodic random table at real coordinates: an analytic texture, nothing resampled."""
    n = table.shape[0]
    iu, iv = np.floor(u), np.floor(v)
    fu, fv = u - iu, v - iv
    iu, iv = iu.astype(np.int64) % n, iv.astype(np.int64) % n
    ju, jv = (iu + 1) % n, (iv + 1) % n
    top = table[iv, iu] * (1 - fu) + table[iv, ju] * fu
    bot = table[jv, iu] * (1 - fu) + table[jv, ju] * fu
    return top * (1 - fv) + bot * fv


def scene(rows, cols, camera, motion, seed=0, far=6.0, near=14.0):
    """-> (image uint8, disparity float32) of the view whose camera is reached from the scene's frame through `motion`
    (X_view = R X + t).  The scene, in the frame of the identity view: the plane Z = Z_far (1 + 0.25 X / W) with W the half
    width it shows at Z_far, and in front of it the patch Z = Z_near over the middle third of the view.  Z_far, Z_near: the
    depths of disparities `far` and `near`.  Every pixel comes from the intersection of its ray with the two surfaces; the
    texture is a function of the point on the surface."""
    fx, fy, cx, cy, baseline = (float(v) for v in camera)
    R = np.asarray(motion[0], np.float64).reshape(3, 3)
    t = np.asarray(motion[1], np.float64).ravel()
    rng = np.random.default_rng(seed)
    tables = [rng.random((64, 64)) for _ in range(3)]
    zf, zn = fx * baseline / far, fx * baseline / near
    half = 0.5 * cols * zf / fx
    u, v = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ R  # R^T applied to the view's rays
    o = -(R.T @ t)
    # patch: Z = zn, |X| < half_n / 3 of the width it shows, |Y| likewise
    lam_n = (zn - o[2]) / ray[..., 2]
    Pn = o + lam_n[..., None] * ray
    wn, hn = 0.5 * cols * zn / fx / 3.0, 0.5 * rows * zn / fy / 2.0
    on_patch = (lam_n > 0) & (np.abs(Pn[..., 0]) < wn) & (np.abs(Pn[..., 1]) < hn)
    # plane: Z - s X = zf with s = 0.25 zf / half
    s = 0.25 * zf / half
    lam_f = (zf - (o[2] - s * o[0])) / (ray[..., 2] - s * ray[..., 0])
    Pf = o + lam_f[..., None] * ray
    P = np.where(on_patch[..., None], Pn, Pf)
    lam = np.where(on_patch, lam_n, lam_f)
    # about 6 pixels per texture cell on either surface, a finer octave on top, a different texture on the patch
    k_f, k_n = fx / zf / 6.0, fx / zn / 6.0
    tex_f = 0.7 * _value_noise(tables[0], P[..., 0] * k_f, P[..., 1] * k_f) + 0.3 * _value_noise(tables[2], P[..., 0] * k_f * 2.7, P[..., 1] * k_f * 2.7)
    tex_n = 0.7 * _value_noise(tables[1], P[..., 0] * k_n + 9.5, P[..., 1] * k_n + 3.5) + 0.3 * _value_noise(tables[2], P[..., 0] * k_n * 2.7, P[..., 1] * k_n * 2.7)
    tex = np.where(on_patch, tex_n, tex_f)
    image = np.clip(np.rint(255.0 * tex), 0, 255).astype(np.uint8)
    # the depth along the view's optical axis is lam (its rays have z = 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        disp = np.where(lam > 0, fx * baseline / lam, 0.0).astype(np.float32)
    return image, disp


# the accuracy scene of tests/test_motion.py and profiles/motion_accuracy.txt: 96x160, from the identity guess
SCENE_TRACK = dict(cell=8, patch_radius=5, search_radius=20, min_score=1)
SCENE_SOLVE = dict(iterations=20, huber_px=1.0, epsilon=1e-10, inlier_px=1.0, min_inliers=30)
SCENE_MOTIONS = ("identity", "baseline", "advance", "yaw", "roll")


def scene_pair(name, seed=0):
    """-> (old image, its disparity, new image, camera, the true motion) at 96x160 under the motion tests/test_reproject.py
    gives that name."""
    from pointcloud_ref import camera_for
    from test_reproject import motions
    rows, cols = 96, 160
    cam = camera_for(rows, cols)
    truth = motions(cam, cam[0] * cam[4] / 6.0)[name]
    old, disp = scene(rows, cols, cam, IDENTITY, seed=seed)
    new, _ = scene(rows, cols, cam, truth, seed=seed)
    return old, disp, new, cam, truth


def seed_share(disp, cam, estimate, truth):
    """Of the pixels > 0 of pm_reproject_disparity's left seed through `estimate`, the share that is within 1 px of the seed
    through `truth` (definition: tests/reproject_ref.py)."""
    import reproject_ref as RR
    a = RR.reproject(disp, cam, estimate[0], estimate[1])["seed_l"]
    b = RR.reproject(disp, cam, truth[0], truth[1])["seed_l"]
    pos = a > 0
    return float(((b > 0) & (np.abs(a - b) <= 1.0))[pos].mean())


def write_accuracy(path):
    """profiles/motion_accuracy.txt: what THE DEFINITION reaches on the accuracy scene; no GPU takes part."""
    lines = ["Accuracy of the definition (tests/motion_ref.py) alone: tools/fuzz_motion.py --accuracy, no GPU takes part.",
             "Scene: 96x160, a textured slanted plane (disparity about 6) with a fronto-parallel patch (disparity 14) in front,",
             "both frames rendered by ray-surface intersection (tools/fuzz_motion.py: scene, seed 0), nothing resampled.",
             "Motions: tests/test_reproject.py: motions(camera, fx * baseline / 6).  Guess: the identity.",
             "Track options %s" % SCENE_TRACK, "Solve options %s" % SCENE_SOLVE, "",
             "motion     records   OK  used  inliers  iterations  rms_px   rotation error [deg]  translation error [m]  |t| [m]"]
    for name in SCENE_MOTIONS:
        old, disp, new, cam, truth = scene_pair(name)
        R, t, info, tr = MR.estimate(old, disp, new, cam, None, SCENE_TRACK, SCENE_SOLVE)
        lines.append("%-10s %7d %4d %5d %8d %11d  %6.4f   %20.3e  %21.3e  %7.4f" % (
            name, len(tr), MR.ok_tracks(tr).sum(), info["n_used"], info["n_inliers"], info["iterations"], info["rms_px"],
            rotation_angle_deg(R, truth[0]), np.linalg.norm(t - truth[1]), np.linalg.norm(truth[1])))
        if name == "yaw":
            share = seed_share(disp, cam, (R, t), truth)
    lines += ["", "Of the pixels > 0 of pm_reproject_disparity's left seed through the estimated motion, the share within 1 px of the",
              "seed through the true motion (definitions: tests/reproject_ref.py, close_radius 1):",
              "seed share (yaw): %.4f" % share, "",
              "tests/test_motion.py asserts twice the recorded errors for the definition, and the recorded share minus 0.02 for the",
              "device; the device result itself is held to the definition bit for bit."]
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def rotation_angle_deg(Ra, Rb):
    """The angle between two rotations in degrees: |Ra - Rb|_F = 2 sqrt(2) sin(angle / 2), which stays exact near 0."""
    d = np.linalg.norm(np.asarray(Ra, np.float64).ravel() - np.asarray(Rb, np.float64).ravel())
    return float(np.degrees(2 * np.arcsin(min(d / (2 * np.sqrt(2)), 1.0))))


# ---- the device against the definition ------------------------------------------------------------------------------------------
def describe(a, b):
    bad = [k for k in range(min(len(a), len(b))) if a[k].tobytes() != b[k].tobytes()]
    return "%d of %d records differ; (k, got, want): %s" % (len(bad), len(b), [(k, a[k], b[k]) for k in bad[:4]])


def check_motion(torch, e, old, disp, new, camera, guess=None, capacity="count", outputs=("tracks", "d_count", "count"),
                 want=None, **opt):
    """One pm_track_features call against the definition.  capacity: an int, or "count" / "count-1" / "count+3" (of the
    definition's count); outputs: which of the three are asked for.  Returns the definition's records."""
    rows, cols = old.shape
    opt = dict(MR.TRACK_DEFAULTS, **opt)
    if want is None:
        want = MR.track(old, disp, new, camera, guess, **opt)
    n = len(want)
    cap = {"count": n, "count-1": max(n - 1, 0), "count+3": n + 3}.get(capacity, capacity)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_old, d_disp, d_new = up(old), up(disp), up(new)
    rec = Guarded(torch, 32 * cap) if "tracks" in outputs and cap > 0 else None
    if rec is None and "d_count" not in outputs and "count" not in outputs:
        outputs = tuple(outputs) + ("count",)  # a call without any output is refused
    cnt = Guarded(torch, 4) if "d_count" in outputs else None
    torch.cuda.synchronize()  # the uploads run on torch's stream, the stage on the handle's: nothing else orders them
    got_n = e.track_features(camera, d_old.data_ptr(), d_disp.data_ptr(), d_new.data_ptr(), rows, cols, guess,
                             capacity=cap if rec else 0, d_tracks=rec.ptr if rec else None, d_count=cnt.ptr if cnt else None,
                             want_count="count" in outputs, **opt)
    e.synchronize()
    if "count" in outputs:
        assert got_n == n, "host count %s, definition %d" % (got_n, n)
    else:
        assert got_n is None
    if cnt:
        assert int(cnt.read(np.int32)[0]) == n, "d_count differs from the definition's %d" % n
    if rec:
        m = min(n, cap)
        got = rec.read(np.uint8, 32 * m).view(MR.TRACK)  # and nothing behind record m was written
        assert got.tobytes() == want[:m].tobytes(), "pm_track_features: " + describe(got, want[:m])
    return want


def check_estimate(torch, e, old, disp, new, camera, guess=None, track_options=None, solve_options=None, want=None):
    """One pm_estimate_motion call against the definition -> the definition's (R, t, info, tracks)."""
    rows, cols = old.shape
    if want is None:
        want = MR.estimate(old, disp, new, camera, guess, track_options, solve_options)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_old, d_disp, d_new = up(old), up(disp), up(new)
    torch.cuda.synchronize()
    R, t, info = e.estimate_motion(camera, d_old.data_ptr(), d_disp.data_ptr(), d_new.data_ptr(), rows, cols, guess,
                                   track_options, solve_options)
    same_motion(R, t, info, *want[:3], "pm_estimate_motion")
    return want


def same_motion(R, t, info, want_R, want_t, want_info, what):
    f64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    assert {k: v for k, v in info.items() if k != "rms_px"} == {k: v for k, v in want_info.items() if k != "rms_px"}, (what, info, want_info)
    assert np.array_equal(f64([info["rms_px"]]), f64([want_info["rms_px"]])), (what, info, want_info)
    assert np.array_equal(f64(R), f64(want_R)) and np.array_equal(f64(t), f64(want_t)), (what, R, want_R, t, want_t)


KINDS = ("noise", "binary", "periodic", "ramp", "scene", "shift")


def images(kind, rng, rows, cols, camera):
    """-> (old, new): "noise" (the new image disturbed by +-9), "binary" (0 / 255, rolled by up to 3), "periodic" (periods
    2 .. 5: SAD and score ties), "ramp" (a constant gradient: flat parabolas), "scene" (rendered, unmoved), "shift" (rendered,
    rolled by up to 4)."""
    if kind == "noise":
        old = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
        new = np.clip(old.astype(np.int64) + rng.integers(-9, 10, (rows, cols)), 0, 255).astype(np.uint8)
    elif kind == "binary":
        old = (rng.integers(0, 2, (rows, cols)) * 255).astype(np.uint8)
        new = np.roll(old, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), (0, 1))
    elif kind == "periodic":
        py, px = int(rng.integers(2, 6)), int(rng.integers(2, 6))
        y, x = np.mgrid[0:rows, 0:cols]
        old = (((y % py) * 37 + (x % px) * 59) % 256).astype(np.uint8)
        new = old.copy()
    elif kind == "ramp":
        y, x = np.mgrid[0:rows, 0:cols]
        old = ((2 * x + y) % 256).astype(np.uint8)
        new = old.copy()
    else:
        old, _ = scene(rows, cols, camera, IDENTITY, seed=int(rng.integers(1 << 30)))
        new = np.roll(old, (int(rng.integers(-4, 5)), int(rng.integers(-4, 5))), (0, 1)) if kind == "shift" else old
    return old, np.ascontiguousarray(new)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-rows", type=int, default=96)
    ap.add_argument("--max-cols", type=int, default=160)
    ap.add_argument("--accuracy", action="store_true", help="write profiles/motion_accuracy.txt from the definition alone and exit")
    a = ap.parse_args()
    if a.accuracy:
        write_accuracy(os.path.join(ROOT, "profiles", "motion_accuracy.txt"))
        return
    import torch
    import pm_ctypes as pm
    rng = np.random.default_rng(a.seed)
    t0, records, oks, valid = time.time(), 0, 0, 0
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        for case in range(a.cases):
            rows, cols = int(rng.integers(1, a.max_rows + 1)), int(rng.integers(1, a.max_cols + 1))
            f = float(rng.uniform(0.8, 3.0) * cols)
            camera = (f, f * float(rng.uniform(0.8, 1.25)), cols / 2 + float(rng.normal(0, 3)), rows / 2 + float(rng.normal(0, 3)),
                      float(rng.uniform(0.02, 0.5)))
            kind = str(rng.choice(KINDS))
            old, new = images(kind, rng, rows, cols, camera)
            disp = random_disp(rng, rows, cols, valid=float(rng.choice([0.3, 0.9, 1.0])), special=float(rng.choice([0.0, 0.1])), hi=30.0)
            how, guess = random_motion(rng, camera, camera[0] * camera[4] / 10.0)
            if rng.random() < 0.4:
                how, guess = "none", None
            opt = dict(cell=int(rng.integers(8, 65)), patch_radius=int(rng.integers(1, 8)), search_radius=int(rng.integers(0, 25)),
                       min_score=int(rng.choice([1, 1000, 10 ** 9])), min_disp=float(rng.choice([0.0, 2.0])),
                       max_disp=float(rng.choice([0.0, 25.0])), max_sad=int(rng.choice([0, 50, 2000])), min_gap=int(rng.choice([0, 1, 40])))
            capacity = rng.choice(["count", "count-1", "count+3", "0"])
            capacity = 0 if capacity == "0" else str(capacity)
            outputs = tuple(k for k in ("tracks", "d_count", "count") if rng.random() < 0.8) or ("count",)
            if outputs == ("tracks",) and capacity == 0:
                outputs = ("tracks", "count")
            what = dict(case=case, rows=rows, cols=cols, camera=camera, images=kind, guess=how, capacity=capacity, outputs=outputs, **opt)
            try:
                want = check_motion(torch, e, old, disp, new, camera, guess, capacity, outputs, **opt)
                records += len(want)
                oks += int(MR.ok_tracks(want).sum())
                sopt = dict(iterations=int(rng.integers(1, 12)), huber_px=float(rng.choice([0.5, 2.0])), min_inliers=6)
                got = check_estimate(torch, e, old, disp, new, camera, guess, opt, sopt)
                valid += got[2]["valid"]
            except AssertionError as err:
                print("MISMATCH", what, err)
                sys.exit(1)
    print("fuzz_motion: %d cases (seed %d), %d records, %d OK, %d valid solves, bit-identical to the definition, %.1f s"
          % (a.cases, a.seed, records, oks, valid, time.time() - t0))


if __name__ == "__main__":
    main()
