"""The organised grid mesh behind the point cloud (include/pm/imaging.h: pm_grid_mesh).

CPU tests pin the definition (tests/mesh_ref.py) against geometry and against itself, and run the kernels' own per-thread
code (csrc/pm_mesh_body.hpp) on the host under ASan / UBSan, the blocks in forward and in reverse order.  GPU tests hold the
kernels to the definition with tolerance 0 -- the vertex streams are pm_point_cloud's arithmetic, the triangle predicate is
comparisons of binary64 differences, and the order of both compactions is arithmetic, not atomics -- with guard bands behind
both capacities."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mesh_ref as MR
import normals_fit_ref as NR
import pointcloud_ref as PR
import speckle_ref as SR
from conftest import GOLDEN, ROOT
from cpp_build import build_host_kernel
from host_run import assert_program_compares, dump_case
from pointcloud_ref import camera_for

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_cloud as FC  # noqa: E402
import fuzz_mesh as FM  # noqa: E402  (check_mesh: the device-against-definition comparison)

gpu = pytest.mark.gpu
MODES = (MR.VERTICES_ALL, MR.VERTICES_REFERENCED)


# ---- 1. the definition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign,diagonal", [(-1.0, 0), (1.0, 1)], ids=["minus_plane", "plus_plane"])
def test_definition_on_an_analytic_plane(sign, diagonal):
    """d = 20 + 0.11 x -/+ 0.07 y at 37x53: every cell is two triangles, every triangle's geometric normal
    (P1 - P0) x (P2 - P0) has Z < 0, and the plane's slope decides the diagonal: along 00-11 the disparity changes by
    0.11 -/+ 0.07, along 10-01 by 0.11 +/- 0.07, and the smaller change wins."""
    rows, cols = 37, 53
    cam = (400.0, 410.0, cols / 2 - 2.3, rows / 2 + 1.7, 0.12)
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    d = (20 + 0.11 * x + sign * 0.07 * y).astype(np.float32)
    for mode in MODES:
        m = MR.grid_mesh(d, cam, max_diff=0.5, vertices=mode)
        assert m["tri_count"] == 2 * 36 * 52 and m["vertex_count"] == rows * cols
        assert m["t0"].all() and m["t1"].all() and (m["diag"] == diagonal).all()
        p = m["xyz"].astype(np.float64)[m["tris"]]
        nz = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])[:, 2]
        assert (nz < 0).all()
        assert np.array_equal(m["index"], np.arange(rows * cols))


def test_definition_cuts_a_step_edge():
    """A step of 2 * max_diff down the middle of a map: no triangle spans it, each side is fully meshed."""
    rows, cols, step, max_diff = 12, 20, 10, 0.5
    d = np.full((rows, cols), 30.0, np.float32)
    d[:, step:] += np.float32(2 * max_diff)
    for mode in MODES:
        m = MR.grid_mesh(d, camera_for(rows, cols), max_diff=max_diff, vertices=mode)
        xs = m["index"][m["tris"]] % cols
        assert ((xs < step).all(axis=1) | (xs >= step).all(axis=1)).all()
        assert m["tri_count"] == 2 * (rows - 1) * (cols - 2) and m["vertex_count"] == rows * cols
        assert not m["t0"][:, step - 1].any() and not m["t1"][:, step - 1].any()
    # the rule is <=: a step of exactly max_diff is no edge
    d[:, step:] = np.float32(30.0 + max_diff)
    assert MR.grid_mesh(d, camera_for(rows, cols), max_diff=max_diff)["tri_count"] == 2 * (rows - 1) * (cols - 1)


def test_definition_vertex_modes_agree():
    """Random quarter-pixel maps with 50 to 90 % valid pixels at strides 1 to 3: the triangles of the two modes name the
    same pixels, the REFERENCED vertices are exactly the pixels the ALL-mode triangles use, and the ALL-mode vertex streams
    are pointcloud_ref.point_cloud's."""
    rng = np.random.default_rng(17)
    seen = set()
    for valid, stride in itertools.product((0.5, 0.7, 0.9), (1, 2, 3)):
        rows, cols = 37, 53
        cam = camera_for(rows, cols)
        d = FM.plateau_disp(rng, rows, cols, valid=valid, special=0.05)
        nrm = rng.normal(size=(rows, cols, 3)).astype(np.float32)
        bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        kw = dict(min_disp=8.5, stride=stride, normal_map=nrm, bgr=bgr)
        a = MR.grid_mesh(d, cam, max_diff=0.5, vertices=MR.VERTICES_ALL, **kw)
        r = MR.grid_mesh(d, cam, max_diff=0.5, vertices=MR.VERTICES_REFERENCED, **kw)
        assert a["tri_count"] == r["tri_count"] > 0
        assert np.array_equal(a["index"][a["tris"]], r["index"][r["tris"]])
        used = np.unique(a["index"][a["tris"]])
        assert np.array_equal(used, r["index"]) and r["vertex_count"] == used.size < a["vertex_count"]
        pc = PR.point_cloud(d, cam, **kw)
        assert pc["count"] == a["vertex_count"]
        for k in ("xyz", "normals", "bgr", "index"):
            assert np.array_equal(FC.bits(a[k]), FC.bits(pc[k])), k
        # truncation: counts stay, streams are prefixes, triangles keep the untruncated numbering
        t = MR.grid_mesh(d, cam, max_diff=0.5, vertices=MR.VERTICES_REFERENCED, vertex_capacity=7, tri_capacity=5, **kw)
        assert (t["vertex_count"], t["tri_count"]) == (r["vertex_count"], r["tri_count"])
        assert np.array_equal(t["index"], r["index"][:7]) and np.array_equal(t["tris"], r["tris"][:5])
        both = a["t0"] & a["t1"]
        seen |= {("two", int(v)) for v in np.unique(a["diag"][both])} | {("one", int(v)) for v in np.unique(a["diag"][a["t0"] ^ a["t1"]])}
    assert seen == {("two", 0), ("two", 1), ("one", 0), ("one", 1)}


def test_definition_specials_never_join():
    """+inf counts (it is > 0) but its difference to anything is inf or NaN: a vertex in ALL mode, never a triangle's."""
    d = np.full((4, 4), 10.0, np.float32)
    d[1, 1] = np.inf
    d[2, 2] = np.nan
    a = MR.grid_mesh(d, camera_for(4, 4), max_diff=1e30, vertices=MR.VERTICES_ALL)
    r = MR.grid_mesh(d, camera_for(4, 4), max_diff=1e30, vertices=MR.VERTICES_REFERENCED)
    assert a["vertex_count"] == 15 and 5 in a["index"] and 5 not in r["index"] and 10 not in a["index"]
    assert a["tri_count"] == r["tri_count"] > 0 and 5 not in a["index"][a["tris"]]
    inf2 = np.full((2, 2), np.inf, np.float32)
    assert MR.grid_mesh(inf2, camera_for(2, 2), max_diff=1e30)["tri_count"] == 0


# ---- 2. the kernels' own per-thread code, run on the host ----------------------------------------------------------------
@pytest.fixture(scope="module")
def host_mesh_exe(tmp_path_factory):
    """tests/cpp/mesh_host_main.cpp: csrc/pm_mesh_body.hpp compiled for the host alone, with the sanitizers."""
    return build_host_kernel(tmp_path_factory.mktemp("meshhost") / "mesh_host_main", "mesh_host_main.cpp")


def _dump_case(path, rng, block, rows, cols, stride, mode, vcap, tcap, reverse):
    """vcap / tcap: "count", "count-1", 0 or a number beyond the count."""
    cam = camera_for(rows, cols)
    disp = FM.plateau_disp(rng, rows, cols, valid=0.75, special=0.08)
    nrm = rng.normal(size=(rows, cols, 3)).astype(np.float32)
    bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    kw = dict(min_disp=8.5, max_range=float(np.float32(cam[0] * cam[4] / 9.0)), stride=stride, max_diff=0.5, vertices=mode,
              normal_map=nrm, bgr=bgr)
    full = MR.grid_mesh(disp, cam, **kw)
    cap = lambda spec, n: max(n, 0) if spec == "count" else max(n - 1, 0) if spec == "count-1" else spec
    vc, tc = cap(vcap, full["vertex_count"]), cap(tcap, full["tri_count"])
    m = MR.grid_mesh(disp, cam, vertex_capacity=vc, tri_capacity=tc, **kw)
    dump_case(path, [rows, cols, *cam, kw["min_disp"], kw["max_range"], stride, kw["max_diff"], mode, vc, tc, block, reverse],
              disp=disp, normals=nrm, bgr=bgr, want_counts=np.array([m["vertex_count"], m["tri_count"]], np.int32),
              **{"want_" + k: m[k] for k in ("xyz", "normals", "bgr", "index", "tris")})
    return m["vertex_count"], m["tri_count"]


def test_kernel_code_on_the_host_equals_the_definition(host_mesh_exe, tmp_path, pm):
    """mesh_value, mesh_cell, mesh_referenced, mesh_store_vertex and mesh_store_triangles over whole maps on the CPU, walked
    block by block as the three launches form them, forwards and backwards: the streams equal the .npy dumps of the
    definition byte for byte, and AddressSanitizer / UBSan see every access into buffers of exactly the size the stage may
    touch.  Shapes without a cell (1x1, 1x9, 9x1), 2x2, 8x8, 37x53 at strides 1 .. 3 and at a stride larger than the image,
    5x300 (two segments of a grid row: a cell straddles their border); both vertex modes; the capacities {count, count - 1,
    0, beyond the count} of vertices and of triangles in every combination."""
    rng = np.random.default_rng(41)
    block = pm.mesh_constants()[0]
    shapes = [(1, 1, 1), (1, 9, 1), (9, 1, 1), (2, 2, 1), (8, 8, 1), (37, 53, 1), (37, 53, 2), (37, 53, 3), (37, 53, 200),
              (5, 300, 1), (5, 600, 2)]
    caps = itertools.cycle(itertools.product(("count", "count-1", 0, 100000), repeat=2))
    vertices = triangles = 0
    k = 0
    for (rows, cols, stride), mode in itertools.product(shapes, MODES):
        for reverse in (0, 1):
            vcap, tcap = next(caps)
            d = str(tmp_path / ("case%d" % k))
            nv, nt = _dump_case(d, rng, block, rows, cols, stride, mode, vcap, tcap, reverse)
            if rows < 2 or cols < 2 or stride == 200:
                assert nt == 0
            vertices, triangles, k = vertices + nv, triangles + nt, k + 1
            r = subprocess.run([host_mesh_exe, d], capture_output=True, text=True)
            assert r.returncode == 0, ((rows, cols, stride, mode, vcap, tcap, reverse), r.stderr[-3000:])
    assert k >= 32 and vertices > 5000 and triangles > 3000  # the 16 capacity combinations came round at least twice
    # the program does compare: one flipped bit in an expectation is a mismatch, not a pass
    d = str(tmp_path / "flipped")
    nv, nt = _dump_case(d, rng, block, 37, 53, 1, MR.VERTICES_REFERENCED, "count", "count", 1)
    assert nt > 100
    assert_program_compares(host_mesh_exe, d, [("want_tris", np.int32, "mesh triangles differs"),
                                               ("want_index", np.int32, "mesh index differs")])


def test_headers_declare_and_the_library_exports_the_mesh_functions(pm):
    text = open(os.path.join(ROOT, "include", "pm", "imaging.h")).read()
    assert "vertex_count > vertex_capacity tells the caller" in text  # the sentence on truncated vertices
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = pm.load()
    assert re.search(r"\bint\s+pm_grid_mesh\s*\(\s*pm_handle\s*\*", text)
    assert "pm_grid_mesh" in pm.EXPORTS and hasattr(lib, "pm_grid_mesh")
    assert "pm_debug_mesh_constants" in pm.EXPORTS and hasattr(lib, "pm_debug_mesh_constants")
    assert "typedef struct pm_mesh_options" in text and "typedef enum pm_mesh_vertices" in text
    assert re.search(r"PM_MESH_VERTICES_ALL\s*=\s*0\s*,\s*PM_MESH_VERTICES_REFERENCED\s*=\s*1", text)
    assert C.sizeof(pm.PmMeshOptions) == 8 and (pm.PM_MESH_VERTICES_ALL, pm.PM_MESH_VERTICES_REFERENCED) == (0, 1)
    per_block, per_pass = pm.mesh_constants()
    assert per_block >= 64 and per_block % 64 == 0 and per_pass >= 64
    assert per_pass == pm.cloud_constants()[1]  # the offsets kernel is the cloud's


# ---- 3. device parity ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        yield e


MAPS = ["all_zero", "all_valid", "checkerboard", "random_mask", "segment_straddle", "more_blocks_than_one_scan_pass"]
MAX_DIFF = 0.5  # against plateau_disp's quarter-pixel values: equal, 0.25 and 0.5 apart join, 0.75 and more are cut


def _mesh_maps(pm):
    """name -> map.  A block is `per_block` items of ONE grid row, so a 20-column map has one block per grid row: with more
    than 3 * per_pass rows even the stride-3 grid has more blocks than one pass of the offsets kernel covers, for the vertex
    scan and for the triangle scan alike.  The three unstructured maps hold every value of fuzz_cloud.SPECIALS."""
    rng = np.random.default_rng(91)
    per_block, per_pass = pm.mesh_constants()
    big_rows, big_cols = 3 * per_pass + 5, 20
    assert big_cols <= per_block and (big_rows + 2) // 3 > per_pass
    checker = np.indices((37, 53)).sum(axis=0) % 2 == 0
    maps = {
        "all_zero": np.zeros((37, 53), np.float32),
        "all_valid": FM.plateau_disp(rng, 37, 53, valid=1.0, special=0.0),
        "checkerboard": np.where(checker, FM.plateau_disp(rng, 37, 53, valid=1.0, special=0.0), 0.0).astype(np.float32),
        "random_mask": FM.plateau_disp(rng, 37, 53, valid=0.7, special=0.05),
        "segment_straddle": FM.plateau_disp(rng, 5, 300, valid=0.95, special=0.02, spread=1.0),
        "more_blocks_than_one_scan_pass": FM.plateau_disp(rng, big_rows, big_cols, valid=0.8, special=0.02),
    }
    assert 300 > per_block  # two segments at stride 1: the cell between items per_block - 1 and per_block straddles them
    for name in ("random_mask", "segment_straddle", "more_blocks_than_one_scan_pass"):
        per_row = (maps[name].shape[1] + 5) // 6  # on the stride-6 grid: every stride of the test sees each of them
        for k, v in enumerate(FC.SPECIALS):
            maps[name][6 * (k // per_row), 6 * (k % per_row)] = v
    return maps


def _assert_not_trivial(want, what):
    """The definition alone emits one-triangle and two-triangle cells on both diagonals: no case passes by being empty."""
    both, one = want["t0"] & want["t1"], want["t0"] ^ want["t1"]
    for d in (0, 1):
        assert (both & (want["diag"] == d)).any() and (one & (want["diag"] == d)).any(), (what, d)
    assert want["vertex_count"] > 0


def test_parity_maps_are_not_trivial(pm):
    """Without a GPU: what the device test asserts about its maps before it compares."""
    for name, disp in _mesh_maps(pm).items():
        rows, cols = disp.shape
        for stride in (1, 2, 3):
            want = MR.grid_mesh(disp, camera_for(rows, cols), min_disp=8.5, stride=stride, max_diff=MAX_DIFF)
            if name == "all_zero":
                assert want["vertex_count"] == want["tri_count"] == 0
            elif name == "checkerboard" and stride != 2:  # (stride 2 sees the one colour only)
                assert want["tri_count"] == 0 and want["vertex_count"] > 0
            elif name != "checkerboard":
                _assert_not_trivial(want, (name, stride))
                zero = MR.grid_mesh(disp, camera_for(rows, cols), min_disp=8.5, stride=stride, max_diff=0.0)
                assert 0 < zero["tri_count"] < want["tri_count"], (name, stride)
        if name in ("random_mask", "segment_straddle", "more_blocks_than_one_scan_pass"):
            for v in FC.SPECIALS:
                assert (FC.bits(disp) == FC.bits(np.array([v], np.float32))[0]).any(), (name, v)


@gpu
@pytest.mark.parametrize("name", MAPS)
def test_grid_mesh_equals_the_definition(pm, engine, name):
    """Strides 1, 2, 3 x both vertex modes x vertex capacity {count, count - 1, 0} x triangle capacity {count, count - 1, 0}
    x {every optional stream absent, every one present}, and max_diff = 0 (only equal disparities join) once per stride and
    mode: counts from the host and from d_counts, every stream equal to the definition, the records at and beyond
    min(count, capacity) still holding their guard pattern."""
    import torch
    disp = _mesh_maps(pm)[name]
    rows, cols = disp.shape
    cam = camera_for(rows, cols)
    rng = np.random.default_rng(5)
    nrm = rng.normal(size=(rows, cols, 3)).astype(np.float32)
    bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    for stride, mode in itertools.product((1, 2, 3), MODES):
        kw = dict(min_disp=8.5, stride=stride, vertices=mode)
        want = MR.grid_mesh(disp, cam, max_diff=MAX_DIFF, normal_map=nrm, bgr=bgr, **kw)
        if name not in ("all_zero", "checkerboard"):
            _assert_not_trivial(want, (name, stride, mode))
        for vcap, tcap in itertools.product(("count", "count-1", 0), repeat=2):
            FM.check_mesh(torch, engine, disp, cam, max_diff=MAX_DIFF, vertex_capacity=vcap, tri_capacity=tcap, outputs=("tris",),
                          want=want, **kw)
            FM.check_mesh(torch, engine, disp, cam, max_diff=MAX_DIFF, vertex_capacity=vcap, tri_capacity=tcap, normal_map=nrm,
                          bgr=bgr, want=want, **kw)
        zero = FM.check_mesh(torch, engine, disp, cam, max_diff=0.0, normal_map=nrm, bgr=bgr, **kw)
        assert zero["tri_count"] <= want["tri_count"]
        if name not in ("all_zero", "checkerboard"):
            assert 0 < zero["tri_count"] < want["tri_count"]
    # no output at all, and no counts on the host: the call only enqueues, d_counts still arrive
    FM.check_mesh(torch, engine, disp, cam, vertex_capacity=7, tri_capacity=7, outputs=(), host_counts=False)
    FM.check_mesh(torch, engine, disp, cam, vertex_capacity=7, tri_capacity=7, outputs=("index",), d_counts=False)
    # the filter's other half: max_range against the point's Z
    FM.check_mesh(torch, engine, disp, cam, max_range=float(np.float32(cam[0] * cam[4] / 9.0)), max_diff=MAX_DIFF,
                  vertices=MR.VERTICES_REFERENCED, outputs=("xyz", "index", "tris"))


@gpu
def test_all_vertices_are_the_point_cloud_s_bytes(engine):
    """PM_MESH_VERTICES_ALL against pm_point_cloud itself on the device: the same count and the same bytes."""
    import torch
    rng = np.random.default_rng(23)
    rows, cols = 37, 300
    disp = FM.plateau_disp(rng, rows, cols, valid=0.7, special=0.1)
    cam = camera_for(rows, cols)
    d = torch.from_numpy(disp).cuda()
    n = engine.point_cloud(cam, d.data_ptr(), rows, cols, 0, min_disp=8.5, stride=2)
    bufs = {k: [FC.Guarded(torch, w * n) for _ in range(2)] for k, w in (("xyz", 12), ("index", 4))}
    assert engine.point_cloud(cam, d.data_ptr(), rows, cols, n, min_disp=8.5, stride=2, d_xyz_out=bufs["xyz"][0].ptr,
                              d_index_out=bufs["index"][0].ptr) == n
    nv, nt = engine.grid_mesh(cam, d.data_ptr(), rows, cols, n, 0, max_diff=0.5, min_disp=8.5, stride=2,
                              d_xyz_out=bufs["xyz"][1].ptr, d_index_out=bufs["index"][1].ptr)
    engine.synchronize()
    assert nv == n > 1000 and nt > 100
    for k, dt in (("xyz", np.uint32), ("index", np.int32)):
        assert np.array_equal(bufs[k][0].read(dt), bufs[k][1].read(dt)), k


@gpu
def test_fuzz_mesh_one_short_seeded_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_mesh.py"), "--cases", "12", "--seed", "4"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@gpu
def test_invalid_arguments_are_named_and_nothing_is_enqueued(pm, engine):
    """PM_ERR_INVALID_ARG with pm_last_error naming the argument; every output keeps its guard pattern."""
    import torch
    rows, cols = 16, 24
    lib, h = engine.lib, engine.h
    disp = torch.full((rows, cols), 10.0, dtype=torch.float32, device="cuda")
    nrm = torch.ones((rows, cols, 3), dtype=torch.float32, device="cuda")
    bgr = torch.ones((rows, cols, 3), dtype=torch.uint8, device="cuda")
    outs = {k: FC.Guarded(torch, w * rows * cols) for k, w in (("xyz", 12), ("normals", 12), ("bgr", 3), ("index", 4),
                                                               ("tris", 24), ("counts", 8))}
    good = camera_for(rows, cols)
    host_counts = (C.c_int * 2)(-5, -6)

    def mesh(cam=good, flt=(0.0, 0.0, 1), opt=(1.0, 0), vcap=rows * cols, tcap=2 * rows * cols, d_disp=disp.data_ptr(),
             d_normals=nrm.data_ptr(), d_bgr=bgr.data_ptr(), rows_=rows, cols_=cols):
        c = pm.cloud_camera(cam)
        f = pm.PmCloudFilter(*flt) if flt is not None else None
        o = pm.PmMeshOptions(*opt) if opt is not None else None
        return lib.pm_grid_mesh(h, C.byref(c) if c is not None else None, C.byref(f) if f is not None else None,
                                C.byref(o) if o is not None else None, d_disp, d_normals, d_bgr, rows_, cols_, vcap, tcap,
                                outs["xyz"].ptr, outs["normals"].ptr, outs["bgr"].ptr, outs["index"].ptr, outs["tris"].ptr,
                                outs["counts"].ptr, host_counts)

    def refused(rc, word, status=None):
        text = lib.pm_last_error(h).decode()
        assert rc == (pm.PM_ERR_INVALID_ARG if status is None else status) and word in text, (rc, word, text)

    refused(mesh(cam=None), "camera")
    for i, name in enumerate(("fx", "fy", "cx", "cy", "baseline")):
        for bad in (np.nan, np.inf, -np.inf):
            cam = list(good)
            cam[i] = bad
            refused(mesh(cam=cam), name)
    refused(mesh(cam=(0.0,) + good[1:]), "fx")
    refused(mesh(cam=(good[0], 0.0) + good[2:]), "fy")
    refused(mesh(flt=None), "filter")
    refused(mesh(opt=None), "options")
    refused(mesh(d_disp=None), "d_disp")
    refused(mesh(flt=(0.0, 0.0, 0)), "stride")
    refused(mesh(flt=(np.nan, 0.0, 1)), "min_disp")
    refused(mesh(flt=(0.0, -1.0, 1)), "max_range")
    for bad in (np.nan, np.inf, -0.5):
        refused(mesh(opt=(bad, 0)), "max_diff")
    for bad in (-1, 2):
        refused(mesh(opt=(1.0, bad)), "vertices")
    refused(mesh(vcap=-1), "vertex_capacity")
    refused(mesh(tcap=-1), "tri_capacity")
    refused(mesh(d_normals=None), "d_normals")
    refused(mesh(d_bgr=None), "d_bgr8")
    refused(mesh(rows_=0), "empty")
    refused(mesh(cols_=-3), "empty")
    # PM_ERR_SIZE: the shape is refused before anything is read (2^15 x 2^15 has more than 2^31 - 1 possible triangles)
    refused(mesh(rows_=1 << 15, cols_=(1 << 16) - 8), "triangles", pm.PM_ERR_SIZE)
    refused(mesh(rows_=1 << 16, cols_=1 << 16), "pixel", pm.PM_ERR_SIZE)
    engine.synchronize()
    for buf in outs.values():
        buf.read(np.uint8, 0)
    assert tuple(host_counts) == (-5, -6)
    # and the same arguments made good do run
    assert mesh() == pm.PM_OK and tuple(host_counts) == (rows * cols, 2 * (rows - 1) * (cols - 1))


@gpu
def test_mesh_scratch_is_owned_by_the_handle(pm):
    """Block counts, totals and the slot map of pm_grid_mesh are ONE handle-owned allocation through csrc/pm_devbuf.hpp: made
    on first use, reused at the same or a smaller size, grown for a larger map, gone with the handle."""
    import torch
    lib = pm.load()
    live = lambda: (lib.pm_debug_live_device_allocations(), lib.pm_debug_live_device_bytes())
    before = live()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        base = live()
        small = torch.full((37, 53), 3.0, dtype=torch.float32, device="cuda")
        large = torch.full((300, 500), 3.0, dtype=torch.float32, device="cuda")
        tris = torch.zeros((2 * 36 * 52, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert e.grid_mesh(camera_for(37, 53), small.data_ptr(), 37, 53, 0, 0) == (37 * 53, 2 * 36 * 52)
        first = live()
        assert first[0] == base[0] + 1 and first[1] >= base[1] + 4 * 37 * 53
        assert e.grid_mesh(camera_for(37, 53), small.data_ptr(), 37, 53, 0, 0, stride=2) == (19 * 27, 2 * 18 * 26)
        assert e.grid_mesh(camera_for(37, 53), small.data_ptr(), 37, 53, 0, tris.shape[0], d_tri_out=tris.data_ptr(),
                           vertices=pm.PM_MESH_VERTICES_REFERENCED) == (37 * 53, 2 * 36 * 52)
        assert live() == first
        assert e.grid_mesh(camera_for(300, 500), large.data_ptr(), 300, 500, 0, 0) == (300 * 500, 2 * 299 * 499)
        grown = live()
        assert grown[0] == first[0] and grown[1] >= first[1] + 4 * (300 * 500 - 37 * 53)
        assert e.grid_mesh(camera_for(37, 53), small.data_ptr(), 37, 53, 0, 0) == (37 * 53, 2 * 36 * 52)
        assert live() == grown
    assert live() == before


@gpu
def test_scalar_match_to_speckles_to_normals_to_mesh(pm):
    """End to end on the golden 376x240 pair: a PM_MODE_SCALAR Match(), then on the device pm_filter_speckles ->
    pm_disparity_normals -> pm_grid_mesh with REFERENCED vertices, normals and triangles.  Each stage equals its definition
    applied to the downloaded map of the stage before."""
    import torch
    z = np.load(os.path.join(GOLDEN, "farmsim_fs1_376x240.npz"))
    l, r = z["left"], z["right"]
    rows, cols = l.shape
    cam = camera_for(rows, cols)
    prm = pm.default_params(1, patchmatch_iters=3, cost_alpha=0.9, sparse_init=1, templ_cols=31, templ_rows=11, max_disp=128,
                            max_matching_cost=0.15)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        dl, _ = e.match(l, r)
        assert (dl > 0).mean() > 0.2
        D = torch.from_numpy(np.ascontiguousarray(dl)).cuda()
        F = torch.zeros_like(D)
        N = torch.zeros((rows, cols, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        e.filter_speckles(D.data_ptr(), rows, cols, 1.0, 50, d_out=F.data_ptr())
        e.disparity_normals(cam, F.data_ptr(), rows, cols, 3, 1.0, 9, d_normals=N.data_ptr())
        e.synchronize()
        filtered, nrm = F.cpu().numpy(), N.cpu().numpy()
        assert np.array_equal(FC.bits(filtered), FC.bits(SR.filter_speckles(dl, 1.0, 50)["out"]))
        assert np.array_equal(FC.bits(nrm), FC.bits(NR.disparity_normals(filtered, cam, 3, 1.0, 9)["normals"]))
        want = FM.check_mesh(torch, e, filtered, cam, max_diff=1.0, vertices=MR.VERTICES_REFERENCED, normal_map=nrm,
                             outputs=("xyz", "normals", "index", "tris"))
    assert want["tri_count"] > 10000 and 0 < want["vertex_count"] < int((filtered > 0).sum())
    assert want["tris"].min() == 0 and want["tris"].max() == want["vertex_count"] - 1
