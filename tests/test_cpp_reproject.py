"""The temporal-seed functions of the C++ host mirror (ocean-perception_amd/host/imaging.hpp: RelativeMotion,
ReprojectDisparity), compiled with plain g++ and driven like a host caller (tests/cpp/reproject_main.cpp): RelativeMotion
agrees with the 4x4 matrix algebra it stands for, and ReprojectDisparity returns, byte for byte, what the definition
(tests/reproject_ref.py) says.  RelativeMotion needs no GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import reproject_ref as RR
from conftest import ROOT
from cpp_build import build_caller

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_reproject as FR  # noqa: E402

ROWS, COLS = 64, 96
CAMERA = (412.7, 398.3, COLS // 2 - 0.3, ROWS // 2 + 0.4, 0.12)  # what reproject_main.cpp sets


@pytest.fixture(scope="module")
def reproject_exe(tmp_path_factory):
    return build_caller(tmp_path_factory.mktemp("cppreproject") / "reproject_main", "reproject_main.cpp")


def _poses():
    old, new = np.eye(4), np.eye(4)
    old[:3, :3], old[:3, 3] = FR.rotation((0.2, 1.0, -0.1), 12.0), (1.5, -0.25, 3.0)
    new[:3, :3], new[:3, 3] = FR.rotation((0.1, 1.0, 0.05), 13.5), (1.52, -0.26, 3.04)
    return old, new


def test_relative_motion_is_the_matrix_algebra(reproject_exe, tmp_path):
    """T_new_old = T_world_new^-1 * T_world_old, against numpy's inverse and against the definition's own helper."""
    old, new = _poses()
    np.stack([old, new]).astype(np.float64).tofile(os.path.join(tmp_path, "poses.f64"))
    r = subprocess.run([reproject_exe, "motion", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "ok motion" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(os.path.join(tmp_path, "motion.f64"), np.float64)
    T = np.linalg.inv(new) @ old
    assert np.abs(got[:9].reshape(3, 3) - T[:3, :3]).max() < 1e-14 and np.abs(got[9:] - T[:3, 3]).max() < 1e-14
    R, t = RR.relative_motion(old, new)
    assert np.abs(got[:9] - R).max() < 1e-15 and np.abs(got[9:] - t).max() < 1e-15
    assert np.abs(got[9:]).max() > 0.01  # the camera did move


@pytest.mark.gpu
def test_reproject_disparity_gives_the_definition(reproject_exe, tmp_path):
    rng = np.random.default_rng(21)
    disp = FR.random_disp(rng, ROWS, COLS, valid=0.9, special=0.05, lo=4.0, hi=16.0)
    disp[20:44, 30:66] += np.float32(10.0)
    R, t = RR.relative_motion(*_poses())
    disp.tofile(os.path.join(tmp_path, "disp.f32"))
    np.concatenate([R, t]).astype(np.float64).tofile(os.path.join(tmp_path, "motion.f64"))
    res = subprocess.run([reproject_exe, "reproject", str(tmp_path), str(ROWS), str(COLS)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.count("refused: ") == 2 and "close_radius" in res.stdout, res.stdout + res.stderr
    want = RR.reproject(disp, CAMERA, R, t, min_disp=1.0, close_radius=2)
    assert (want["seed_l"] > 0).mean() >= 0.25 and (want["seed_r"] > 0).mean() >= 0.25
    assert not np.array_equal(want["seed_l"], disp)  # the motion does move the map
    load = lambda name, dt: np.fromfile(os.path.join(tmp_path, name), dt)
    assert np.array_equal(FR.bits(load("seed_l.f32", np.float32)), FR.bits(want["seed_l"].ravel()))
    assert np.array_equal(FR.bits(load("seed_r.f32", np.float32)), FR.bits(want["seed_r"].ravel()))
    assert np.array_equal(load("counts.i32", np.int32), want["counts"])
    assert np.array_equal(FR.bits(load("right_only.f32", np.float32)), FR.bits(want["seed_r"].ravel()))
    assert np.array_equal(load("right_only_counts.i32", np.int32), [-1, -1])
