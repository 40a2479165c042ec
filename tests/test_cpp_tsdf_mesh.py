"""TsdfVolume::Mesh of the C++ host mirror (ocean-perception_amd/host/imaging.hpp), compiled with plain g++ and driven like a
host caller (tests/cpp/tsdf_mesh_main.cpp): host maps in, a TriangleMesh out, on the matcher's own handle, byte for byte what the
definition (tests/tsdf_mesh_ref.py) says of the definition's volume (tests/tsdf_ref.py), and WritePly's file of it read back."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_mesh_ref as MR
import tsdf_ref as TR
from cpp_build import build_caller
from test_cpp_mesh import read_ply
from test_tsdf import IDENT
from test_tsdf_mesh import bits, case_grid


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_caller(tmp_path_factory.mktemp("cpptsdfmesh") / "tsdf_mesh_main", "tsdf_mesh_main.cpp")


def test_the_caller_compiles_against_the_mirror(exe):
    """No GPU: the header declares Mesh, MeshDevice and TsdfMeshOptions, the library exports what they call, and the program says
    how it wants to be called."""
    assert subprocess.run([exe]).returncode == 2


@pytest.mark.gpu
def test_mesh_gives_the_definition_and_its_ply_reads_back(exe, tmp_path):
    rows, cols = 48, 80
    grid = case_grid("37x21x13")
    cam = (90.0, 90.0, 40.0, 24.0, 0.12)
    y, x = np.mgrid[:rows, :cols]
    depth = 1.0 + 0.24 * (0.5 + 0.3 * np.sin(0.2 * x) * np.cos(0.15 * y))
    maps = np.stack([(cam[0] * cam[4] / depth).astype(np.float32)] * 2)
    maps[1][:, 40:] = 0
    vol = TR.clear(grid)
    for d in maps:
        vol = TR.integrate(grid, vol, d, cam, *IDENT)["voxels"]
    want = MR.mesh(grid, vol, 2.0)
    assert 100 < want["counts"][0] < MR.mesh(grid, vol, 0.0)["counts"][0] and want["counts"][1] > 100
    put = lambda name, a, dt: np.ascontiguousarray(a, dt).tofile(os.path.join(tmp_path, name))
    put("grid.f64", [grid["nx"], grid["ny"], grid["nz"], *grid["origin"], grid["voxel"], grid["trunc"], grid["max_weight"]], np.float64)
    put("camera.f64", cam, np.float64)
    put("disp.f32", maps, np.float32)
    put("options.f32", [2.0], np.float32)
    res = subprocess.run([exe, str(tmp_path), str(rows), str(cols), "2"], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.count("refused: ") == 2 and "min_weight" in res.stdout, res.stdout + res.stderr
    load = lambda name, dt: np.fromfile(os.path.join(tmp_path, name), dt)
    assert tuple(load("counts.i32", np.int32)) == tuple(want["counts"]) * 2
    assert np.array_equal(load("xyz.f32", np.uint32), bits(want["xyz"]).ravel())
    assert np.array_equal(load("plain_xyz.f32", np.uint32), bits(want["xyz"]).ravel())
    assert np.array_equal(load("normals.f32", np.uint32), bits(want["normals"]).ravel())
    assert np.array_equal(load("tris.i32", np.int32).reshape(-1, 3), want["tris"])
    assert tuple(load("empty.i32", np.int32)) == (0, 0)
    for name, fields in (("mesh", ("x", "y", "z", "nx", "ny", "nz")), ("plain", ("x", "y", "z"))):
        head, v, f = read_ply(os.path.join(tmp_path, name + ".ply"))
        assert v.dtype.names == fields and (len(v), len(f)) == tuple(want["counts"])
        assert np.array_equal(np.stack([v[k] for k in "xyz"], -1).view(np.uint32), bits(want["xyz"]))
        assert np.array_equal(f, want["tris"])
    assert np.array_equal(np.stack([v[k] for k in "xyz"], -1), want["xyz"])
    head, v, f = read_ply(os.path.join(tmp_path, "mesh.ply"))
    assert np.array_equal(np.stack([v[k] for k in ("nx", "ny", "nz")], -1).view(np.uint32), bits(want["normals"]))
