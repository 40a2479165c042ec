"""FuseDisparity of the C++ host mirror (ocean-perception_amd/host/imaging.hpp), compiled with plain g++ and driven like a
host caller (tests/cpp/fuse_main.cpp): host images in, host images out, on the matcher's own handle, and byte for byte what
the definition (tests/fuse_ref.py) says."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fuse_ref as FU
from conftest import ROOT
from cpp_build import build_caller
from test_fuse import fuse_case

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_fuse as FF  # noqa: E402

ROWS, COLS = 64, 96
CAMERA = (412.7, 398.3, COLS // 2 - 0.3, ROWS // 2 + 0.4, 0.12)  # what fuse_main.cpp sets


@pytest.fixture(scope="module")
def fuse_exe(tmp_path_factory):
    return build_caller(tmp_path_factory.mktemp("cppfuse") / "fuse_main", "fuse_main.cpp")


def test_the_caller_compiles_against_the_mirror(fuse_exe):
    """No GPU: the header declares FuseDisparity and FuseOptions, the library exports it, and the program says how it wants to
    be called."""
    assert subprocess.run([fuse_exe]).returncode == 2


@pytest.mark.gpu
def test_fuse_disparity_gives_the_definition(fuse_exe, tmp_path):
    cur, _, sources, mots, _ = fuse_case(ROWS, COLS, ("identity", "yaw", "advance"), cam=CAMERA)
    cur = cur.copy()
    cur.ravel()[:FF.SPECIALS.size] = FF.SPECIALS
    rng = np.random.default_rng(31)
    weights = [FF.random_weight(rng, ROWS, COLS), FF.random_weight(rng, ROWS, COLS)]
    cur.tofile(os.path.join(tmp_path, "disp.f32"))
    np.stack(sources).astype(np.float32).tofile(os.path.join(tmp_path, "sources.f32"))
    np.stack(weights).tofile(os.path.join(tmp_path, "weights.f32"))
    np.concatenate([np.concatenate([np.asarray(R).ravel(), np.asarray(t).ravel()]) for R, t in mots]).astype(np.float64).tofile(
        os.path.join(tmp_path, "motions.f64"))
    res = subprocess.run([fuse_exe, str(tmp_path), str(ROWS), str(COLS), "3"], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.count("refused: ") == 3 and "fill_min_sources" in res.stdout, res.stdout + res.stderr
    want = FU.fuse(cur, sources, CAMERA, mots, weights[0], [weights[1], None, None], 0.75, 1, 1, 8, 2, 0.75)
    valid, kept, fused, filled = want["counts"]
    assert valid > 0.25 * ROWS * COLS and 0.5 * valid < fused <= kept <= valid and filled > 50
    load = lambda name, dt: np.fromfile(os.path.join(tmp_path, name), dt)
    assert np.array_equal(load("out.f32", np.uint32), FF.bits(want["out"]).ravel())
    assert np.array_equal(load("count.u8", np.uint8), want["count"].ravel())
    assert np.array_equal(load("spread.f32", np.uint32), FF.bits(want["spread"]).ravel())
    assert np.array_equal(load("flags.u8", np.uint8), want["flags"].ravel())
    assert np.array_equal(load("counts.i32", np.int32), want["counts"])
    plain = FU.fuse(cur, sources, CAMERA, mots, None, None, 0.75, 1, 1, 8, 0, 0.75)
    assert plain["counts"][3] == 0 and not np.array_equal(FF.bits(plain["out"]), FF.bits(want["out"]))
    assert np.array_equal(load("out_only.f32", np.uint32), FF.bits(plain["out"]).ravel())
    assert np.array_equal(load("out_only_counts.i32", np.int32), plain["counts"])
