"""AlignColorDisparity and TsdfVolume::AlignColor of the C++ host mirror (ocean-perception_amd/host/imaging.hpp) and
pm_align_sums_blend, compiled with plain g++ and driven like a host caller (tests/cpp/align_color_main.cpp): host images in,
motions out, on the matcher's own handle, and bit for bit what the definition (tests/align_photo_ref.py) and the C ABI say."""
import os
import subprocess

import numpy as np
import pytest

import align_photo_ref as AP
import align_ref as AR
import tsdf_color_ref as TC
import tsdf_ref as TR
from cpp_build import build_caller
from test_align import CAM, COLS, GRID, RAY, ROWS, Z0, motions, perturbed, seeded_sums
from test_align_photo import BAND, OPT, chain_pose, image_of, render_plane, to_bytes, view


@pytest.fixture(scope="module")
def color_exe(tmp_path_factory):
    return build_caller(tmp_path_factory.mktemp("cppaligncolor") / "align_color_main", "align_color_main.cpp")


def test_the_caller_compiles_against_the_mirror(color_exe):
    """No GPU: the header declares AlignColorDisparity, TsdfVolume::AlignColor and AlignColorOptions, the library exports what the
    program calls, and the program says how it wants to be called."""
    assert subprocess.run([color_exe]).returncode == 2


def _flat_info(info):
    g = info["geo"]
    return np.array([g["valid"], g["n_model"], g["n_gate"], g["n_used"], g["iterations"], g["rms_px"], *g["H"], info["n_photo_model"],
                     info["n_photo_gate"], info["n_photo_used"], info["rms_levels"], *info["H"]], np.float64)


def _flat(m):
    return np.concatenate([np.asarray(m[0], np.float64).ravel(), np.asarray(m[1], np.float64).ravel()])


@pytest.mark.gpu
def test_the_mirror_gives_the_definition_and_the_c_abi(color_exe, tmp_path):
    """The degenerate plane under the 2-degree yaw, float and byte images; then the tracking leg: the coloured volume sees the plane
    from one pose of the chain, the new frame is the next."""
    rng = np.random.default_rng(9)
    put = lambda name, a, dt: np.ascontiguousarray(a, dt).tofile(os.path.join(tmp_path, name))
    load = lambda name: np.fromfile(os.path.join(tmp_path, name), np.float64)
    same = lambda a, b: np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))
    truth = motions(CAM, Z0)["yaw"]
    guess = perturbed(truth)
    pose, pose_new = chain_pose(1), chain_pose(2)
    records = []
    for _ in range(2):
        H, g = seeded_sums(rng)
        records.append(dict(H=np.array(H), g=np.array(g), rr=float(rng.uniform(0, 9)), n_model=int(rng.integers(5000)),
                            n_gate=int(rng.integers(5000)), n_used=int(rng.integers(5000))))
    flat_record = lambda r: [*r["H"], *r["g"], r["rr"], r["n_model"], r["n_gate"], r["n_used"]]
    put("camera.f64", CAM, np.float64)
    put("options.f64", [OPT[k] for k in ("min_disp", "max_diff", "huber_px", "iterations", "epsilon", "min_used", "huber_levels", "lam")], np.float64)
    put("guess.f64", _flat(guess), np.float64)
    put("grid.f64", [GRID["nx"], GRID["ny"], GRID["nz"], *GRID["origin"], GRID["voxel"], GRID["trunc"], GRID["max_weight"]], np.float64)
    put("ray.f32", [RAY["min_range"], RAY["max_range"], RAY["step"], RAY["min_weight"]], np.float32)
    put("band.f32", [BAND], np.float32)
    put("pose.f64", _flat(pose), np.float64)
    put("sums.f64", [*flat_record(records[0]), *flat_record(records[1]), 0.07], np.float64)

    def run(dm, nm, im, dn, inew):
        put("disp_model.f32", dm, np.float32)
        put("normals_model.f32", nm, np.float32)
        put("bgr_model.f32", im, np.float32)
        put("disp_new.f32", dn, np.float32)
        put("bgr_new.f32", inew, np.float32)
        put("bgr8_new.u8", to_bytes(inew), np.uint8)
        res = subprocess.run([color_exe, str(tmp_path), str(ROWS), str(COLS)], capture_output=True, text=True)
        assert res.returncode == 0 and res.stdout.count("refused: ") == 3 and "lambda" in res.stdout, res.stdout + res.stderr

    dm, nm, im = view("plane")
    dn, _, inew = view("plane", "yaw")
    run(dm, nm, im, dn, inew)
    for image, motion, info in ((inew, "motion.f64", "info.f64"), (to_bytes(inew), "motion8.f64", "info8.f64"), (to_bytes(inew), "abi_motion.f64", "abi_info.f64")):
        want, winfo = AP.align_color(CAM, OPT, guess, dm, nm, im, dn, image)
        assert winfo["geo"]["valid"] == 1 and winfo["geo"]["iterations"] > 1
        assert same(load(motion), _flat(want)) and same(load(info), _flat_info(winfo)), motion
    want = AP.blend(records[0], records[1], 0.07)
    assert same(load("blend.f64"), flat_record(want))

    d_pose, d_next = render_plane(pose), render_plane(pose_new)
    im_pose, im_next = image_of(pose, d_pose), image_of(pose_new, d_next)
    run(d_pose, nm, im_pose, d_next, im_next)
    first = TC.integrate(GRID, TR.clear(GRID), TC.clear(GRID), d_pose, im_pose, CAM, *pose, band=BAND)
    ray = TR.raycast(GRID, first["voxels"], CAM, pose[0], pose[1], ROWS, COLS, **RAY)
    model = TC.color_map(GRID, first["colors"], ray["disp"], CAM, pose[0], pose[1])["bgr"]
    M, tinfo = AP.align_color(CAM, OPT, None, ray["disp"], ray["normals"], model, d_next, to_bytes(im_next))
    assert tinfo["geo"]["valid"] == 1
    assert same(load("tracked.f64"), _flat(AR.compose(M, pose))) and same(load("tracked_info.f64"), _flat_info(tinfo))
