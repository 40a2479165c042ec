"""Points, plane-mode normals and the compacted cloud behind the range stages (include/pm/imaging.h: pm_backproject,
pm_planes_normals, pm_point_cloud).

CPU tests pin the definition (tests/pointcloud_ref.py) against geometry and against pm_disp_to_range's formula, and run
the kernels' own per-thread code (csrc/pm_cloud_body.hpp) on the host under ASan / UBSan.  GPU tests
hold the kernels to the definition with tolerance 0 -- every operation of the definition is one IEEE rounding, the build
uses -ffp-contract=off and correctly rounded binary32 division and sqrt, and the order of the compacted cloud is
arithmetic, not atomics -- with guard bands around every output."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pointcloud_ref as PR
from conftest import GOLDEN, ROOT
from cpp_build import build_host_kernel
from host_run import assert_program_compares, dump_case
from pointcloud_ref import camera_for

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_cloud as FC  # noqa: E402  (check_backproject / check_cloud: the device-against-definition comparisons)

gpu = pytest.mark.gpu


# ---- 1. the definition ------------------------------------------------------------------------------------------------
def test_definition_against_an_analytic_plane():
    """A 3-D plane n0 . P = h seen by a camera with fx != fy renders to the disparity plane d(x, y) = a (x - cx) + b (y - cy)
    + fx B n0z / h with a = B n0x / h and b = fx B n0y / (fy h).  Every normal of the definition must be -n0 and every point
    must satisfy the plane equation, to 1e-5 relative: the project's tolerance for its float stages, and what is left of
    binary32 after a, b and d were rounded to it."""
    rows, cols = 48, 64
    fx, fy, cx, cy, B = 420.0, 390.0, 31.3, 24.6, 0.12
    n0 = np.array([0.3, -0.2, 1.0])
    n0 /= np.linalg.norm(n0)
    h = 2.0
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    a, b = B * n0[0] / h, fx * B * n0[1] / (fy * h)
    d = (a * (x - cx) + b * (y - cy) + fx * B * n0[2] / h).astype(np.float32)
    assert (d > 10).all()
    planes = np.stack([np.full((rows, cols), a, np.float32), np.full((rows, cols), b, np.float32), d])
    cam = (fx, fy, cx, cy, B)
    nrm = PR.normals(planes, cam)
    assert nrm.dtype == np.float32 and np.abs(nrm.astype(np.float64) + n0).max() <= 1e-5
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=2) - 1).max() <= 1e-6
    pts = PR.backproject(d, cam).astype(np.float64)
    assert np.abs(pts @ n0 - h).max() <= 1e-5 * h
    # the mask: zero normals exactly where the map is not > 0, whatever the state holds there
    mask = d.copy()
    mask[::3, ::2] = 0.0
    mask[1, 1] = np.nan
    masked = PR.normals(planes, cam, mask)
    off = ~(mask > 0)
    assert (masked[off] == 0).all() and np.array_equal(masked[~off], nrm[~off]) and off.sum() > 500
    # the state's own z: not > 0 gives no normal
    planes[2, 5, :] = 0.0
    planes[2, 6, :] = -3.0
    assert (PR.normals(planes, cam)[5:7] == 0).all()


def test_definition_z_is_the_range_of_disp_to_range():
    """The Z channel equals (float)(fx * baseline / (double)d), pm_disp_to_range's value, bit for bit; 0 where d is not > 0."""
    rng = np.random.default_rng(3)
    d = FC.random_disp(rng, 37, 53, valid=0.8, special=0.15)
    cam = camera_for(37, 53)
    z = PR.backproject(d, cam)[:, :, 2]
    ok = d > 0
    with np.errstate(over="ignore"):
        want = np.where(ok, (np.float64(cam[0]) * np.float64(cam[4]) / np.where(ok, d, 1).astype(np.float64)).astype(np.float32),
                        np.float32(0))
    assert np.array_equal(FC.bits(z), FC.bits(want)) and ok.sum() > 1000 and (~ok).sum() > 100
    assert np.isinf(z).any()  # a subnormal disparity: the range overflows binary32, the point is still defined
    # the cloud takes points unchanged from the organised definition, in row-major order
    pc = PR.point_cloud(d, cam, min_disp=5.0, max_range=4.0, stride=2, capacity=40)
    assert pc["count"] > 40 and len(pc["index"]) == 40 and (np.diff(pc["index"]) > 0).all()
    ys, xs = np.divmod(pc["index"], 53)
    assert (ys % 2 == 0).all() and (xs % 2 == 0).all() and (d[ys, xs] >= 5).all()
    assert np.array_equal(pc["xyz"], PR.backproject(d, cam)[ys, xs]) and (pc["xyz"][:, 2] <= 4.0).all()


# ---- 2. the kernels' own per-thread code, run on the host ----------------------------------------------------------------
@pytest.fixture(scope="module")
def host_cloud_exe(tmp_path_factory):
    """tests/cpp/cloud_host_main.cpp: csrc/pm_cloud_body.hpp compiled for the host alone, with the sanitizers."""
    return build_host_kernel(tmp_path_factory.mktemp("cloudhost") / "cloud_host_main", "cloud_host_main.cpp")


def _dump_case(path, rng, rows, cols, shift, min_disp, max_range, stride, capacity):
    cam = camera_for(rows, cols)
    disp = FC.random_disp(rng, rows, cols, valid=0.7, special=0.15)
    planes = np.stack([rng.choice(np.array([-1.0, 1.0, 0.0, 0.37, -0.004], np.float32), (rows, cols)),
                       rng.choice(np.array([-1.0, 1.0, 0.0, 0.25], np.float32), (rows, cols)),
                       rng.choice(np.array([0.0, -2.0, 40.0, 12.5, 3.0, np.nan], np.float32), (rows, cols))])
    bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    nrm = PR.normals(planes, cam, disp)
    count = PR.point_cloud(disp, cam, min_disp, max_range, stride)["count"]
    cap = 0 if capacity == "zero" else max(count + capacity, 0) if capacity <= 0 else capacity
    pc = PR.point_cloud(disp, cam, min_disp, max_range, stride, cap, nrm, bgr)
    dump_case(path, [rows, cols, *cam, min_disp, max_range, stride, cap, shift], disp=disp, planes=planes, bgr=bgr,
              want_xyz=PR.backproject(disp, cam), want_normals=nrm, want_count=np.array([pc["count"]], np.int32),
              **{"want_cloud_" + k: pc[k] for k in ("xyz", "normals", "bgr", "index")})
    return pc["count"], cap


def test_kernel_code_on_the_host_equals_the_definition(host_cloud_exe, tmp_path):
    """backproject_four (what every thread of k_backproject runs), cloud_normal (k_planes_normals) and cloud_item +
    cloud_store (the count and scatter launches) over whole maps on the CPU: points, normals and the compacted streams equal
    the .npy dumps of the definition byte for byte, and AddressSanitizer / UBSan see every access into buffers of exactly
    the size the stage may touch.  Shapes: 8x8, the odd 37x53 at an aligned and an unaligned destination, a width below one
    thread's four pixels, 64x300; strides 1 .. 3; capacity = count, count - 1, 0 and beyond the count."""
    rng = np.random.default_rng(31)
    # rows, cols, shift (floats), min_disp, max_range, stride, capacity (<= 0: relative to the count; "zero": 0)
    cases = [(8, 8, 0, 0.0, 0.0, 1, 0), (37, 53, 0, 0.0, 0.0, 1, 0), (37, 53, 1, 5.0, 0.0, 2, -1), (37, 53, 3, 0.0, 3.0, 3, 0),
             (5, 3, 2, 0.0, 0.0, 1, 1000), (64, 300, 0, 20.0, 8.0, 1, -1), (1, 1, 1, 0.0, 0.0, 1, 0), (9, 7, 0, 0.0, 0.0, 2, 5),
             (16, 24, 0, 0.0, 0.0, 1, "zero")]
    counted = 0
    for k, c in enumerate(cases):
        d = str(tmp_path / ("case%d" % k))
        count, cap = _dump_case(d, rng, *c)
        counted += count
        r = subprocess.run([host_cloud_exe, d], capture_output=True, text=True)
        assert r.returncode == 0, (c, r.stderr[-3000:])
    assert counted > 3000
    # the program does compare: one flipped bit in an expectation is a mismatch, not a pass
    assert_program_compares(host_cloud_exe, str(tmp_path / "case1"), [("want_cloud_index", np.int32, "cloud index differs")])


def test_headers_declare_and_the_library_exports_the_cloud_functions(pm):
    text = open(os.path.join(ROOT, "include", "pm", "imaging.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = pm.load()
    for name in ("pm_backproject", "pm_planes_normals", "pm_point_cloud"):
        assert re.search(r"\bint\s+%s\s*\(\s*pm_handle\s*\*" % name, text), name
        assert name in pm.EXPORTS and hasattr(lib, name), name
    assert "typedef struct pm_cloud_camera" in text and "typedef struct pm_cloud_filter" in text
    assert C.sizeof(pm.PmCloudCamera) == 40 and C.sizeof(pm.PmCloudFilter) == 12
    per_block, per_pass = pm.cloud_constants()
    assert per_block >= 64 and per_block % 64 == 0 and per_pass >= 64


# ---- 3. device parity ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        yield e


@gpu
@pytest.mark.parametrize("rows,cols,offset", [(8, 8, 0), (37, 53, 0), (64, 300, 0), (37, 53, 1)],
                         ids=["8x8", "37x53", "64x300", "37x53_unaligned"])
def test_backproject_equals_the_definition(engine, rows, cols, offset):
    """Values include 0, -0.0, negatives, NaN, +inf and subnormals; offset 1: d_xyz one float past a 16-byte boundary, so
    every store takes the narrow path.  The bytes on either side of the output keep their pattern."""
    import torch
    rng = np.random.default_rng(rows * 1000 + cols)
    disp = FC.random_disp(rng, rows, cols, valid=0.7, special=0.2)
    disp.ravel()[:FC.SPECIALS.size] = FC.SPECIALS  # each of them at least once
    got = FC.check_backproject(torch, engine, disp, camera_for(rows, cols), offset)
    # Z is pm_disp_to_range's value bit for bit
    cam = camera_for(rows, cols)
    d = torch.from_numpy(disp).cuda()
    r = torch.empty_like(d)
    engine.disp_to_range(d.data_ptr(), rows, cols, cam[0], cam[4], r.data_ptr())
    engine.synchronize()
    assert np.array_equal(FC.bits(got[:, :, 2]), FC.bits(r.cpu().numpy()))


def _cloud_maps(pm):
    """name -> map.  The last shape has more blocks than one pass of the offsets kernel covers: the library reports the
    items per block (256) and the block counts per pass (1024), so at stride 1 a map of 512 columns needs more than 512
    rows: 517 of them are 1034 blocks, ten into the second pass (strides 2 and 3 stay within one pass)."""
    rng = np.random.default_rng(77)
    per_block, per_pass = pm.cloud_constants()
    big_cols = 512
    big_rows = per_block * per_pass // big_cols + 5
    assert big_rows * big_cols > per_block * per_pass
    checker = np.indices((37, 53)).sum(axis=0) % 2 == 0
    return {
        "all_zero": np.zeros((37, 53), np.float32),
        "all_valid": rng.uniform(1.0, 90.0, (37, 53)).astype(np.float32),
        "checkerboard": np.where(checker, rng.uniform(1.0, 90.0, (37, 53)), 0.0).astype(np.float32),
        "random_mask": FC.random_disp(rng, 37, 53, valid=0.5, special=0.1),
        "more_blocks_than_one_scan_pass": FC.random_disp(rng, big_rows, big_cols, valid=0.6, special=0.02),
    }


@gpu
@pytest.mark.parametrize("name", ["all_zero", "all_valid", "checkerboard", "random_mask", "more_blocks_than_one_scan_pass"])
def test_point_cloud_equals_the_definition(pm, engine, name):
    """Strides 1, 2, 3 x {no filter, min_disp, max_range} x capacity {count, count - 1, 0} x {every optional stream absent,
    every one present}: count from the host and from d_count, d_index_out strictly increasing, every stream equal to the
    definition, and the slots at and beyond min(count, capacity) still holding their guard pattern."""
    import torch
    disp = _cloud_maps(pm)[name]
    rows, cols = disp.shape
    cam = camera_for(rows, cols)
    rng = np.random.default_rng(5)
    nrm = rng.normal(size=(rows, cols, 3)).astype(np.float32)
    bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    z_mid = float(np.float32(cam[0] * cam[4] / 20.0))
    counts = []
    for stride in (1, 2, 3):
        for flt in (dict(), dict(min_disp=20.0), dict(max_range=z_mid)):
            for capacity in ("count", "count-1", 0):
                counts.append(FC.check_cloud(torch, engine, disp, cam, stride=stride, capacity=capacity, outputs=("xyz",), **flt))
                FC.check_cloud(torch, engine, disp, cam, stride=stride, capacity=capacity, normal_map=nrm, bgr=bgr, **flt)
    if name == "all_zero":
        assert counts == [0] * len(counts)
    else:
        # counts[stride index * 9 + filter index * 3 + capacity index]: each filter and each stride drops some pixels
        assert counts[0] > counts[3] > 0 and counts[0] > counts[6] > 0 and counts[0] > counts[9] > counts[18] > 0
    # no output at all, and no count on the host: the call only enqueues, d_count still arrives
    FC.check_cloud(torch, engine, disp, cam, capacity=7, outputs=(), host_count=False)
    FC.check_cloud(torch, engine, disp, cam, capacity=7, outputs=("index",), d_count=False)


@gpu
def test_fuzz_cloud_one_short_seeded_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_cloud.py"), "--cases", "12", "--seed", "4"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _planes_params(pm, f16, patch=5, iters=1, **kw):
    return pm.default_params(0, patch=patch, patchmatch_iters=iters, mode=pm.PM_MODE_PLANES, state_dtype=f16, **kw)


def _normals_on_device(torch, e, pair, cam, disp, rows, cols):
    out = FC.Guarded(torch, 12 * rows * cols)
    d = torch.from_numpy(disp).cuda() if disp is not None else None
    e.planes_normals(pair, cam, d.data_ptr() if d is not None else None, rows, cols, out.ptr)
    e.synchronize()
    return out.read(np.float32).reshape(rows, cols, 3)


@gpu
@pytest.mark.parametrize("f16", [0, 1], ids=["f32", "f16"])
def test_planes_normals_of_installed_planes(pm, f16):
    """Hand-made planes written with pm_planes_write at 16x24 and 37x53 -- slopes at +-plane_slope_max included, z = 0 and
    steep planes whose nz is negative -- against the definition applied to what pm_planes_read returns (the f16 state's
    rounding included), without and with a mask map."""
    import torch
    rng = np.random.default_rng(8 + f16)
    prm = _planes_params(pm, f16, max_disp=40)
    smax = float(prm.plane_slope_max)
    with pm.Engine(prm, max_rows=64, max_cols=96) as e:
        for rows, cols in ((16, 24), (37, 53)):
            img = torch.from_numpy(rng.integers(0, 256, (2, rows, cols), dtype=np.uint8)).cuda()
            e.planes_begin(1, img[0].data_ptr(), img[1].data_ptr(), rows, cols)
            planes = np.zeros((4, rows, cols), np.float32)
            planes[0] = rng.choice(np.array([-smax, smax, 0.0, 0.999, -0.5, 0.0371], np.float32), (rows, cols))
            planes[1] = rng.choice(np.array([-smax, smax, 0.0, 0.25, -0.0113], np.float32), (rows, cols))
            planes[2] = rng.choice(np.array([0.0, 40.0, 39.99, 12.5, 3.0, 0.7], np.float32), (rows, cols))
            planes[3] = 1.0
            e.planes_write(0, 0, planes)
            state = e.planes_read(0, 0)
            if not f16:
                assert np.array_equal(state[:3], planes[:3])
            cam = camera_for(rows, cols)
            want = PR.normals(state, cam)
            got = _normals_on_device(torch, e, 0, cam, None, rows, cols)
            assert np.array_equal(FC.bits(got), FC.bits(want)), (rows, cols)
            zero = (got == 0).all(axis=2)
            assert np.array_equal(zero, ~(state[2] > 0)) and 0 < zero.sum() < zero.size
            assert np.abs(np.linalg.norm(got[~zero].astype(np.float64), axis=1) - 1).max() <= 1e-6
            assert (got[:, :, 2] > 0).any() and (got[:, :, 2] < 0).any()  # steep planes: both signs of nz occur
            mask = FC.random_disp(rng, rows, cols, valid=0.5, special=0.2)
            got = _normals_on_device(torch, e, 0, cam, mask, rows, cols)
            assert np.array_equal(FC.bits(got), FC.bits(PR.normals(state, cam, mask))), (rows, cols, "masked")
            # the state is that of this size: another size, or a pair the handle does not hold, is refused
            out = FC.Guarded(torch, 12 * rows * cols)
            for pair, r_, c_ in ((0, rows, cols + 1), (1, rows, cols)):
                with pytest.raises(pm.PmError) as ei:
                    e.planes_normals(pair, cam, None, r_, c_, out.ptr)
                assert ei.value.status == pm.PM_ERR_STATE
            e.synchronize()
            out.read(np.uint8, 0)


@gpu
@pytest.mark.parametrize("f16", [0, 1], ids=["f32", "f16"])
def test_planes_normals_after_a_real_match(pm, f16):
    """A plane-mode pm_match_device on the 64x96 pair of tests/golden/planes_64x96.npz: the normals masked by its d_disp_l
    equal the definition on pm_planes_read + that map and are zero exactly where the map is; then the whole chain into a
    compacted cloud with normals and colour."""
    import torch
    g = np.load(os.path.join(GOLDEN, "planes_64x96.npz"))
    rows, cols = 64, 96
    cam = camera_for(rows, cols)
    L, R = torch.from_numpy(g["left"]).cuda(), torch.from_numpy(g["right"]).cuda()
    DL, DR = torch.zeros((rows, cols), dtype=torch.float32, device="cuda"), torch.zeros((rows, cols), dtype=torch.float32,
                                                                                       device="cuda")
    with pm.Engine(_planes_params(pm, f16, patch=7, iters=3, max_disp=24), max_rows=rows, max_cols=cols) as e:
        e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, None, None, DL.data_ptr(), DR.data_ptr())
        out = FC.Guarded(torch, 12 * rows * cols)
        e.planes_normals(0, cam, DL.data_ptr(), rows, cols, out.ptr)  # same stream: ordered behind the match
        e.synchronize()
        dl = DL.cpu().numpy()
        assert np.array_equal(dl, g["disp_l_f%d" % (16 if f16 else 32)])
        got = out.read(np.float32).reshape(rows, cols, 3)
        state = e.planes_read(0, 0)
        assert np.array_equal(FC.bits(got), FC.bits(PR.normals(state, cam, dl)))
        zero = (got == 0).all(axis=2)
        assert np.array_equal(zero, dl == 0) and 0 < zero.sum() < zero.size
        bgr = np.stack([g["left"], g["left"] // 2, 255 - g["left"]], axis=-1)
        n = FC.check_cloud(torch, e, dl, cam, min_disp=1.0, stride=1, normal_map=got, bgr=bgr)
        assert n == int((dl >= 1.0).sum()) > 1000


@gpu
def test_planes_normals_refuses_a_scalar_mode_handle(pm, engine):
    import torch
    out = FC.Guarded(torch, 12 * 16 * 24)
    with pytest.raises(pm.PmError) as ei:
        engine.planes_normals(0, camera_for(16, 24), None, 16, 24, out.ptr)
    assert ei.value.status == pm.PM_ERR_STATE and "PM_MODE_PLANES" in str(ei.value)
    engine.synchronize()
    out.read(np.uint8, 0)
    # a plane-mode handle that has not matched yet holds no state either
    with pm.Engine(_planes_params(pm, 0), max_rows=64, max_cols=96) as e:
        with pytest.raises(pm.PmError) as ei:
            e.planes_normals(0, camera_for(16, 24), None, 16, 24, out.ptr)
        assert ei.value.status == pm.PM_ERR_STATE


@gpu
def test_invalid_arguments_are_named_and_nothing_is_enqueued(pm, engine):
    """PM_ERR_INVALID_ARG with pm_last_error naming the argument; every output keeps its guard pattern."""
    import torch
    rows, cols = 16, 24
    lib, h = engine.lib, engine.h
    disp = torch.full((rows, cols), 10.0, dtype=torch.float32, device="cuda")
    nrm = torch.ones((rows, cols, 3), dtype=torch.float32, device="cuda")
    bgr = torch.ones((rows, cols, 3), dtype=torch.uint8, device="cuda")
    outs = {k: FC.Guarded(torch, w * rows * cols) for k, w in (("xyz", 12), ("normals", 12), ("bgr", 3), ("index", 4), ("count", 4))}
    good = camera_for(rows, cols)
    host_count = C.c_int(-5)

    def cloud(cam, flt=(0.0, 0.0, 1), capacity=rows * cols, d_normals=nrm.data_ptr(), d_bgr=bgr.data_ptr()):
        c = pm.cloud_camera(cam)
        f = pm.PmCloudFilter(*flt)
        return lib.pm_point_cloud(h, C.byref(c) if c is not None else None, C.byref(f), disp.data_ptr(), d_normals, d_bgr, rows,
                                  cols, capacity, outs["xyz"].ptr, outs["normals"].ptr, outs["bgr"].ptr, outs["index"].ptr,
                                  outs["count"].ptr, C.byref(host_count))

    def backproject(cam):
        c = pm.cloud_camera(cam)
        return lib.pm_backproject(h, C.byref(c) if c is not None else None, disp.data_ptr(), rows, cols, outs["xyz"].ptr)

    def normals(cam):
        c = pm.cloud_camera(cam)
        return lib.pm_planes_normals(h, 0, C.byref(c) if c is not None else None, None, rows, cols, outs["normals"].ptr)

    def refused(rc, word):
        text = lib.pm_last_error(h).decode()
        assert rc == pm.PM_ERR_INVALID_ARG and word in text, (rc, word, text)

    for call in (cloud, backproject, normals):
        refused(call(None), "camera")
        for i, name in enumerate(("fx", "fy", "cx", "cy", "baseline")):
            for bad in (np.nan, np.inf, -np.inf):
                cam = list(good)
                cam[i] = bad
                refused(call(cam), name)
        refused(call((0.0,) + good[1:]), "fx")
        refused(call((good[0], 0.0) + good[2:]), "fy")
    refused(cloud(good, flt=(0.0, 0.0, 0)), "stride")
    refused(cloud(good, flt=(0.0, 0.0, -3)), "stride")
    refused(cloud(good, capacity=-1), "capacity")
    refused(cloud(good, d_normals=None), "d_normals")
    refused(cloud(good, d_bgr=None), "d_bgr8")
    refused(cloud(good, flt=(np.nan, 0.0, 1)), "min_disp")
    refused(cloud(good, flt=(0.0, -1.0, 1)), "max_range")
    engine.synchronize()
    for buf in outs.values():
        buf.read(np.uint8, 0)
    assert host_count.value == -5
    # and the same arguments made good do run
    assert cloud(good) == pm.PM_OK and host_count.value == rows * cols


@gpu
def test_block_offset_scratch_is_owned_by_the_handle(pm):
    """The block counts of pm_point_cloud are ONE handle-owned allocation through csrc/pm_devbuf.hpp: made on first use,
    reused at the same size, grown for a larger map, gone with the handle."""
    import torch
    lib = pm.load()
    live = lambda: (lib.pm_debug_live_device_allocations(), lib.pm_debug_live_device_bytes())
    before = live()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        base = live()
        small = torch.full((37, 53), 3.0, dtype=torch.float32, device="cuda")
        large = torch.full((300, 500), 3.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert e.point_cloud(camera_for(37, 53), small.data_ptr(), 37, 53, 0) == 37 * 53
        first = live()
        assert first[0] == base[0] + 1 and first[1] > base[1]
        assert e.point_cloud(camera_for(37, 53), small.data_ptr(), 37, 53, 0, stride=2) == 19 * 27
        assert live() == first
        assert e.point_cloud(camera_for(300, 500), large.data_ptr(), 300, 500, 0) == 300 * 500
        grown = live()
        assert grown[0] == first[0] and grown[1] > first[1]
        assert e.point_cloud(camera_for(37, 53), small.data_ptr(), 37, 53, 0) == 37 * 53
        assert live() == grown
    assert live() == before
