"""FilterSpeckles of the C++ host mirror (ocean-perception_amd/host/imaging.hpp), compiled with plain g++ and driven like a
host caller (tests/cpp/speckle_main.cpp): what it returns is, byte for byte, what the definition (tests/speckle_ref.py)
says for the same map."""
import os
import subprocess
import sys

import numpy as np
import pytest

import speckle_ref as SR
from conftest import ROOT
from cpp_build import build_caller

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_cloud as FC  # noqa: E402
import fuzz_normals as FN  # noqa: E402

ROWS, COLS = 37, 153  # three tiles wide and three high, none of them whole


@pytest.fixture(scope="module")
def speckle_exe(tmp_path_factory):
    return build_caller(tmp_path_factory.mktemp("cppspeckle") / "speckle_main", "speckle_main.cpp")


def _input(tmp_path):
    disp = FN.run_map(np.random.default_rng(29), ROWS, COLS, valid=0.8, special=0.05)
    disp.tofile(os.path.join(tmp_path, "disp.f32"))
    return disp


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_speckle_mirror_builds_with_gxx_and_fails_loudly_without_gpu(speckle_exe, tmp_path):
    _input(tmp_path)
    r = subprocess.run([speckle_exe, str(tmp_path), str(ROWS), str(COLS)], capture_output=True, text=True)
    assert r.returncode == 10 and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_speckle_mirror_gives_the_bytes_of_the_definition(speckle_exe, tmp_path):
    disp = _input(tmp_path)
    res = subprocess.run([speckle_exe, str(tmp_path), str(ROWS), str(COLS)], capture_output=True, text=True)
    assert res.returncode == 0 and "refused: pm_filter_speckles" in res.stdout and "max_size" in res.stdout, res.stdout + res.stderr
    load = lambda name, dt: np.fromfile(os.path.join(tmp_path, name), dt)
    want = SR.filter_speckles(disp, 1.0, 100)
    assert np.array_equal(FC.bits(load("out.f32", np.float32).reshape(ROWS, COLS)), FC.bits(want["out"]))
    assert np.array_equal(load("labels.i32", np.int32).reshape(ROWS, COLS), want["labels"])
    assert load("removed.i32", np.int32)[0] == want["removed"] > 0 and (want["sizes"] > 100).any()
    want = SR.filter_speckles(disp, 0.25, 3)
    assert np.array_equal(FC.bits(load("out_small.f32", np.float32).reshape(ROWS, COLS)), FC.bits(want["out"]))
