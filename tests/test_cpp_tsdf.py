"""TsdfVolume of the C++ host mirror (ocean-perception_amd/host/imaging.hpp), compiled with plain g++ and driven like a host
caller (tests/cpp/tsdf_main.cpp): host images in, host images out, on the matcher's own handle, and byte for byte what the
definition (tests/tsdf_ref.py) says."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tsdf_ref as TR
from conftest import ROOT
from cpp_build import build_caller
from test_tsdf import tsdf_case

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_tsdf as FT  # noqa: E402


@pytest.fixture(scope="module")
def tsdf_exe(tmp_path_factory):
    return build_caller(tmp_path_factory.mktemp("cpptsdf") / "tsdf_main", "tsdf_main.cpp")


def test_the_caller_compiles_against_the_mirror(tsdf_exe):
    """No GPU: the header declares TsdfVolume and its option structs, the library exports what it calls, and the program says
    how it wants to be called."""
    assert subprocess.run([tsdf_exe]).returncode == 2


@pytest.mark.gpu
def test_tsdf_volume_gives_the_definition(tsdf_exe, tmp_path):
    rows, cols = 37, 53
    args, _ = tsdf_case("37x21x13", "37x53", ("identity", "yaw", "roll"), ray_name="yaw")
    grid, steps, ray = args["grid"], args["steps"], args["ray"]
    w0 = FT.random_weight(np.random.default_rng(31), rows, cols)
    steps = [(steps[0][0], steps[0][1], w0)] + list(steps[1:])
    want = FT.reference(grid, TR.clear(grid), steps, args["camera"], args["ray_pose"], rows, cols, ray)
    put = lambda name, a, dt: np.ascontiguousarray(a, dt).tofile(os.path.join(tmp_path, name))
    put("grid.f64", [grid["nx"], grid["ny"], grid["nz"], *grid["origin"], grid["voxel"], grid["trunc"], grid["max_weight"]], np.float64)
    put("camera.f64", args["camera"], np.float64)
    put("disp.f32", np.stack([s[0] for s in steps]), np.float32)
    put("weights.f32", w0, np.float32)
    put("poses.f64", np.concatenate([np.concatenate([np.asarray(R).ravel(), np.asarray(t).ravel()])
                                     for R, t in [s[1] for s in steps] + [args["ray_pose"]]]), np.float64)
    put("ray.f32", [ray["min_range"], ray["max_range"], ray["step"], ray["min_weight"]], np.float32)
    res = subprocess.run([tsdf_exe, str(tmp_path), str(rows), str(cols), "3"], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.count("refused: ") == 4 and "step" in res.stdout, res.stdout + res.stderr
    assert all(c[1] > 1000 for c in want["counts"]) and want["ray"]["counts"][0] > 100
    load = lambda name, dt: np.fromfile(os.path.join(tmp_path, name), dt)
    assert np.array_equal(load("volume.f32", np.uint32), FT.bits(want["volumes"][-1]).ravel())
    assert np.array_equal(load("counts.i32", np.int32), np.stack(want["counts"]).ravel())
    assert np.array_equal(load("disp_out.f32", np.uint32), FT.bits(want["ray"]["disp"]).ravel())
    assert np.array_equal(load("normals.f32", np.uint32), FT.bits(want["ray"]["normals"]).ravel())
    assert np.array_equal(load("map_only.f32", np.uint32), FT.bits(want["ray"]["disp"]).ravel())
    assert tuple(load("hits.i32", np.int32)) == (want["ray"]["counts"][0],) * 2
    assert (load("cleared.f32", np.uint32) == 0).all() and load("cleared.f32", np.uint32).size == 2 * 37 * 21 * 13
