"""AlignDisparity, ComposeMotion and TsdfVolume::Align of the C++ host mirror (ocean-perception_amd/host/imaging.hpp), compiled with
plain g++ and driven like a host caller (tests/cpp/align_main.cpp): host images in, motions out, on the matcher's own handle, and
bit for bit what the definition (tests/align_ref.py, tests/tsdf_ref.py) and the C ABI say."""
import os
import subprocess

import numpy as np
import pytest

import align_ref as AR
import tsdf_ref as TR
from cpp_build import build_caller
from test_align import CAM, COLS, GRID, OPT, RAY, ROWS, Z0, model_view, motions, perturbed, pose_on_arc, relative, render


@pytest.fixture(scope="module")
def align_exe(tmp_path_factory):
    return build_caller(tmp_path_factory.mktemp("cppalign") / "align_main", "align_main.cpp")


def test_the_caller_compiles_against_the_mirror(align_exe):
    """No GPU: the header declares AlignDisparity, ComposeMotion, TsdfVolume::Align and AlignOptions, the library exports what it
    calls, and the program says how it wants to be called."""
    assert subprocess.run([align_exe]).returncode == 2


def _flat_info(info):
    return np.array([info["valid"], info["n_model"], info["n_gate"], info["n_used"], info["iterations"], info["rms_px"], *info["H"]], np.float64)


def _flat(m):
    return np.concatenate([np.asarray(m[0], np.float64).ravel(), np.asarray(m[1], np.float64).ravel()])


@pytest.mark.gpu
def test_the_mirror_gives_the_definition_and_the_c_abi(align_exe, tmp_path):
    dm, nm = model_view()
    truth = motions(CAM, Z0)["yaw"]
    guess = perturbed(truth)
    dn = render(truth)
    # the tracking leg: the volume sees the model map from a pose on the arc, the new frame is a degree further on
    pose, pose_new = pose_on_arc(1.0), pose_on_arc(2.0)
    d_pose = render(pose)
    d_next = render(pose_new)
    put = lambda name, a, dt: np.ascontiguousarray(a, dt).tofile(os.path.join(tmp_path, name))
    put("camera.f64", CAM, np.float64)
    put("options.f64", [OPT[k] for k in ("min_disp", "max_diff", "huber_px", "iterations", "epsilon", "min_used")], np.float64)
    put("guess.f64", _flat(guess), np.float64)
    put("grid.f64", [GRID["nx"], GRID["ny"], GRID["nz"], *GRID["origin"], GRID["voxel"], GRID["trunc"], GRID["max_weight"]], np.float64)
    put("ray.f32", [RAY["min_range"], RAY["max_range"], RAY["step"], RAY["min_weight"]], np.float32)
    put("pose.f64", _flat(pose), np.float64)
    load = lambda name: np.fromfile(os.path.join(tmp_path, name), np.float64)
    same = lambda a, b: np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))

    # one run per leg: AlignDisparity wants (model, normals, new); Align wants the volume's own view as the model map
    put("disp_model.f32", dm, np.float32)
    put("normals_model.f32", nm, np.float32)
    put("disp_new.f32", dn, np.float32)
    res = subprocess.run([align_exe, str(tmp_path), str(ROWS), str(COLS)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.count("refused: ") == 3 and "min_used" in res.stdout, res.stdout + res.stderr
    want, winfo = AR.align(CAM, OPT, guess, dm, nm, dn)
    assert winfo["valid"] == 1 and winfo["iterations"] > 1
    assert same(load("motion.f64"), _flat(want)) and same(load("info.f64"), _flat_info(winfo))
    assert same(load("abi_motion.f64"), _flat(want)) and same(load("abi_info.f64"), _flat_info(winfo))
    assert same(load("composed.f64"), _flat(AR.compose(want, pose)))

    put("disp_model.f32", d_pose, np.float32)
    put("disp_new.f32", d_next, np.float32)
    res = subprocess.run([align_exe, str(tmp_path), str(ROWS), str(COLS)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    vol = TR.integrate(GRID, TR.clear(GRID), d_pose, CAM, *pose)["voxels"]
    ray = TR.raycast(GRID, vol, CAM, pose[0], pose[1], ROWS, COLS, **RAY)
    M, tinfo = AR.align(CAM, OPT, None, ray["disp"], ray["normals"], d_next)
    assert tinfo["valid"] == 1
    tracked = AR.compose(M, pose)
    assert same(load("tracked.f64"), _flat(tracked)) and same(load("tracked_info.f64"), _flat_info(tinfo))
    # and it is a tracker: closer to the new frame's pose than the guess it started from
    err = lambda p: np.abs(_flat(relative(p, pose_new)) - _flat(AR.IDENTITY)).max()
    assert err(tracked) < 0.5 * err(pose)
