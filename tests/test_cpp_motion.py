"""TrackFeatures, SolveMotion and EstimateMotion of the C++ host mirror (ocean-perception_amd/host/imaging.hpp), compiled with
plain g++ and driven like a host caller (tests/cpp/motion_caller_main.cpp): host images in, records and motions out, on the
matcher's own handle, and byte for byte what the definition (tests/motion_ref.py) and the C ABI give."""
import os
import subprocess

import numpy as np
import pytest

import motion_ref as MR
from cpp_build import build_caller
from test_motion import SCENE_SOLVE, SCENE_TRACK, scene_estimate, scene_pair

ROWS, COLS = 96, 160  # the accuracy scene; its camera is what motion_caller_main.cpp sets


@pytest.fixture(scope="module")
def motion_exe(tmp_path_factory):
    return build_caller(tmp_path_factory.mktemp("cppmotion") / "motion_caller_main", "motion_caller_main.cpp")


def test_the_caller_compiles_against_the_mirror(motion_exe):
    """No GPU: the header declares the three functions and their option structs, the library exports them, and the program says
    how it wants to be called."""
    assert subprocess.run([motion_exe]).returncode == 2


@pytest.mark.gpu
def test_the_mirror_gives_the_definition_and_the_c_abi(motion_exe, tmp_path, pm):
    import torch
    old, disp, new, cam, truth = scene_pair("yaw")
    assert old.shape == (ROWS, COLS) and SCENE_TRACK == dict(cell=8, patch_radius=5, search_radius=20, min_score=1)
    assert SCENE_SOLVE == dict(iterations=20, huber_px=1.0, epsilon=1e-10, inlier_px=1.0, min_inliers=30)
    old.tofile(os.path.join(tmp_path, "old.u8"))
    new.tofile(os.path.join(tmp_path, "new.u8"))
    disp.tofile(os.path.join(tmp_path, "disp.f32"))
    res = subprocess.run([motion_exe, str(tmp_path), str(ROWS), str(COLS)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.count("refused: ") == 4, res.stdout + res.stderr
    assert "search_radius" in res.stdout and "pm_solve_motion" in res.stdout and "sizes differ" in res.stdout
    R, t, info, tracks = scene_estimate("yaw")
    load = lambda name, dt: np.fromfile(os.path.join(tmp_path, name), dt)
    assert load("tracks.bin", np.uint8).tobytes() == tracks.tobytes() and info["valid"] == 1
    want = np.concatenate([R, t]).view(np.uint64)
    want_info = [info[k] for k in ("valid", "n_tracks", "n_used", "n_inliers", "iterations")]
    for stem in ("solved", "estimated"):
        assert np.array_equal(load(stem + ".f64", np.uint64), want), stem
        assert load(stem + "_info.i32", np.int32).tolist() == want_info, stem
        assert load(stem + "_rms.f64", np.uint64)[0] == np.array([info["rms_px"]]).view(np.uint64)[0], stem
    # and the C ABI, called directly, gives the same
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_old, d_disp, d_new = up(old), up(disp), up(new)
    torch.cuda.synchronize()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        got = e.estimate_motion(cam, d_old.data_ptr(), d_disp.data_ptr(), d_new.data_ptr(), ROWS, COLS, None, SCENE_TRACK, SCENE_SOLVE)
    assert np.array_equal(np.concatenate([got[0], got[1]]).view(np.uint64), want) and got[2] == info
    assert MR.ok_tracks(tracks).sum() >= 30
