"""The mesh functions of the C++ host mirror (ocean-perception_amd/host/imaging.hpp: MakeGridMesh, WritePly), compiled with
plain g++ and driven like a host caller (tests/cpp/mesh_main.cpp): MakeGridMesh returns, byte for byte, what the definition
(tests/mesh_ref.py) says, and WritePly's files read back with numpy -- header, counts and bytes.  WritePly needs no GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_ref as MR
from conftest import ROOT
from cpp_build import build_caller

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_cloud as FC  # noqa: E402
import fuzz_mesh as FM  # noqa: E402

ROWS, COLS = 64, 96
CAMERA = (412.7, 398.3, COLS // 2 - 0.3, ROWS // 2 + 0.4, 0.12)  # what mesh_main.cpp sets


@pytest.fixture(scope="module")
def mesh_exe(tmp_path_factory):
    return build_caller(tmp_path_factory.mktemp("cppmesh") / "mesh_main", "mesh_main.cpp")


def read_ply(path):
    """-> (header lines, vertex records as a structured array, faces [t][3] int32); asserts the layout WritePly promises."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")[:-1]
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0" and head[-1] == "end_header"
    assert head[2].startswith("element vertex ")
    n = int(head[2].split()[2])
    face_at = [i for i, line in enumerate(head) if line.startswith("element face ")]
    assert len(face_at) == 1 and head[face_at[0] + 1] == "property list uchar int vertex_indices" and face_at[0] + 3 == len(head)
    t = int(head[face_at[0]].split()[2])
    fields = []
    for line in head[3:face_at[0]]:
        kind, typ, name = line.split()
        assert kind == "property" and typ in ("float", "uchar")
        fields.append((name, "<f4" if typ == "float" else "u1"))
    vt = np.dtype(fields)
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert len(raw) == end + n * vt.itemsize + t * ft.itemsize
    verts = np.frombuffer(raw, vt, n, end)
    faces = np.frombuffer(raw, ft, t, end + n * vt.itemsize)
    assert (faces["n"] == 3).all()
    return head, verts, faces["v"]


def test_write_ply_reads_back(mesh_exe, tmp_path):
    """No device: a hand-made mesh, with and without normals and colour, and an empty one."""
    r = subprocess.run([mesh_exe, "ply", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "ok ply" in r.stdout and "refused: WritePly" in r.stdout, r.stdout + r.stderr
    k = np.arange(4)
    xyz = np.stack([0.5 * (k & 1), -0.25 * (k >> 1), 1.0 + k], axis=1).astype(np.float32)
    for name, names in (("plain", ("x", "y", "z")), ("normals", ("x", "y", "z", "nx", "ny", "nz")),
                        ("full", ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"))):
        head, v, f = read_ply(os.path.join(tmp_path, name + ".ply"))
        assert v.dtype.names == names and len(v) == 4
        assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], axis=1), xyz)
        assert np.array_equal(f, [[0, 2, 3], [0, 3, 1]])
        if "nx" in names:
            assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], axis=1),
                                  np.stack([0 * k, 0.125 * k, -1 + 0 * k], axis=1).astype(np.float32))
        if "red" in names:  # the cloud's bytes are B G R
            assert np.array_equal(v["blue"], 10 + k) and np.array_equal(v["green"], 20 + k) and np.array_equal(v["red"], 30 + k)
    head, v, f = read_ply(os.path.join(tmp_path, "empty.ply"))
    assert len(v) == 0 and len(f) == 0 and head[2] == "element vertex 0"


@pytest.mark.gpu
def test_make_grid_mesh_gives_the_definition(mesh_exe, tmp_path):
    rng = np.random.default_rng(12)
    disp = FM.plateau_disp(rng, ROWS, COLS, valid=0.85, special=0.05)
    nrm = rng.normal(size=(ROWS, COLS, 3)).astype(np.float32)
    bgr = rng.integers(0, 256, (ROWS, COLS, 3), dtype=np.uint8)
    for name, a in (("disp.f32", disp), ("normals.f32", nrm), ("bgr.u8", bgr)):
        np.ascontiguousarray(a).tofile(os.path.join(tmp_path, name))
    res = subprocess.run([mesh_exe, "mesh", str(tmp_path), str(ROWS), str(COLS)], capture_output=True, text=True)
    assert res.returncode == 0 and "refused: pm_grid_mesh" in res.stdout, res.stdout + res.stderr
    load = lambda name, dt, shape: np.fromfile(os.path.join(tmp_path, name), dt).reshape(shape)
    want = MR.grid_mesh(disp, CAMERA, min_disp=8.5, stride=2, max_diff=0.5, vertices=MR.VERTICES_REFERENCED, normal_map=nrm,
                        bgr=bgr)
    assert want["tri_count"] > 100 and want["vertex_count"] > 100
    got = {"xyz": load("ref_xyz.f32", np.float32, (-1, 3)), "normals": load("ref_normals.f32", np.float32, (-1, 3)),
           "bgr": load("ref_bgr.u8", np.uint8, (-1, 3)), "index": load("ref_index.i32", np.int32, (-1,)),
           "tris": load("ref_tris.i32", np.int32, (-1, 3))}
    for k in got:
        assert np.array_equal(FC.bits(got[k]), FC.bits(want[k])), k
    # the file of that mesh
    head, v, f = read_ply(os.path.join(tmp_path, "ref.ply"))
    assert v.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
    assert np.array_equal(FC.bits(np.stack([v["x"], v["y"], v["z"]], axis=1)), FC.bits(want["xyz"]))
    assert np.array_equal(FC.bits(np.stack([v["nx"], v["ny"], v["nz"]], axis=1)), FC.bits(want["normals"]))
    assert np.array_equal(np.stack([v["blue"], v["green"], v["red"]], axis=1), want["bgr"])
    assert np.array_equal(f, want["tris"])
    want = MR.grid_mesh(disp, CAMERA, max_diff=0.5, vertices=MR.VERTICES_ALL)
    assert np.array_equal(FC.bits(load("all_xyz.f32", np.float32, (-1, 3))), FC.bits(want["xyz"]))
    assert np.array_equal(load("all_index.i32", np.int32, (-1,)), want["index"])
    assert np.array_equal(load("all_tris.i32", np.int32, (-1, 3)), want["tris"])
