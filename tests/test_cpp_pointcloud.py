"""The point-cloud functions of the C++ host mirror (ocean-perception_amd/host/imaging.hpp: Backproject, MakePointCloud,
PlaneNormals), compiled with plain g++ and driven like a host caller (tests/cpp/pointcloud_main.cpp): what they return is,
byte for byte, what the C ABI calls return (pm_backproject, pm_point_cloud, pm_planes_normals through the binding) and what
the definition (tests/pointcloud_ref.py) says."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pointcloud_ref as PR
from conftest import ROOT
from cpp_build import build_caller

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_cloud as FC  # noqa: E402

ROWS, COLS = 64, 96
CAMERA = (412.7, 398.3, COLS // 2 - 0.3, ROWS // 2 + 0.4, 0.12)  # what pointcloud_main.cpp sets


@pytest.fixture(scope="module")
def cloud_exe(tmp_path_factory):
    return build_caller(tmp_path_factory.mktemp("cppcloud") / "pointcloud_main", "pointcloud_main.cpp")


def _inputs(tmp_path, synth):
    rng = np.random.default_rng(12)
    disp = FC.random_disp(rng, ROWS, COLS, valid=0.7, special=0.1)
    bgr = rng.integers(0, 256, (ROWS, COLS, 3), dtype=np.uint8)
    p = synth.make_pair(7, rows=ROWS, cols=COLS, n_points=40, dilate_factor=2)
    for name, a in (("disp.f32", disp), ("bgr.u8", bgr), ("left.u8", p["left"]), ("right.u8", p["right"])):
        np.ascontiguousarray(a).tofile(os.path.join(tmp_path, name))
    return disp, bgr


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_cloud_mirror_builds_with_gxx_and_fails_loudly_without_gpu(cloud_exe, tmp_path, synth):
    _inputs(tmp_path, synth)
    r = subprocess.run([cloud_exe, str(tmp_path), str(ROWS), str(COLS)], capture_output=True, text=True)
    assert r.returncode == 10 and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_cloud_mirror_gives_the_bytes_of_the_c_abi(cloud_exe, tmp_path, synth, pm):
    import torch
    disp, bgr = _inputs(tmp_path, synth)
    res = subprocess.run([cloud_exe, str(tmp_path), str(ROWS), str(COLS)], capture_output=True, text=True)
    assert res.returncode == 0 and "refused: pm_planes_normals" in res.stdout, res.stdout + res.stderr
    load = lambda name, dt, shape: np.fromfile(os.path.join(tmp_path, name), dt).reshape(shape)
    xyz = load("xyz.f32", np.float32, (ROWS, COLS, 3))
    cloud = {"xyz": load("cloud_xyz.f32", np.float32, (-1, 3)), "bgr": load("cloud_bgr.u8", np.uint8, (-1, 3)),
             "index": load("cloud_index.i32", np.int32, (-1,))}
    # the C ABI through the binding, on the same inputs
    with pm.Engine(pm.default_params(0, patch=5), max_rows=ROWS, max_cols=COLS) as e:
        assert np.array_equal(FC.bits(FC.check_backproject(torch, e, disp, CAMERA)), FC.bits(xyz))
        n = FC.check_cloud(torch, e, disp, CAMERA, min_disp=5.0, stride=2, bgr=bgr, outputs=("xyz", "bgr", "index"))
    want = PR.point_cloud(disp, CAMERA, min_disp=5.0, stride=2, bgr=bgr)  # what check_cloud held the C ABI to
    assert n == want["count"] == len(cloud["index"]) > 300
    for k in cloud:
        assert np.array_equal(FC.bits(cloud[k]), FC.bits(want[k])), k
    # the plane-mode matcher: normals of the state its Match() left, masked by its left map, and the cloud made of both
    match_l = load("match_l.f32", np.float32, (ROWS, COLS))
    planes = load("planes.f32", np.float32, (4, ROWS, COLS))
    normals = load("normals.f32", np.float32, (ROWS, COLS, 3))
    assert np.array_equal(FC.bits(normals), FC.bits(PR.normals(planes, CAMERA, match_l)))
    zero = (normals == 0).all(axis=2)
    assert np.array_equal(zero, match_l == 0) and 0 < zero.sum() < zero.size
    want = PR.point_cloud(match_l, CAMERA, normal_map=normals)
    assert want["count"] == int((~zero).sum())
    assert np.array_equal(FC.bits(load("ncloud_xyz.f32", np.float32, (-1, 3))), FC.bits(want["xyz"]))
    assert np.array_equal(FC.bits(load("ncloud_normals.f32", np.float32, (-1, 3))), FC.bits(want["normals"]))
    assert np.array_equal(load("ncloud_index.i32", np.int32, (-1,)), want["index"])
