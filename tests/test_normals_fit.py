"""Normals for scalar-mode maps: the windowed, edge-aware plane fit behind the point-cloud stages (include/pm/imaging.h:
pm_disparity_normals).

CPU tests pin the definition (tests/normals_fit_ref.py) against an analytic plane, against central differences on a
run-quantised plane (what a scalar-mode match leaves) and at its edge rules, and run the kernel's own staging and per-pixel
code (csrc/pm_normals_fit_body.hpp) on the host under ASan / UBSan.  GPU tests hold the kernel to the definition with
tolerance 0 -- every operation of the definition is one IEEE rounding in a fixed order and the build uses
-ffp-contract=off -- with guard bands around every output."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import normals_fit_ref as NR
import pointcloud_ref as PR
from conftest import GOLDEN, ROOT
from cpp_build import build_host_kernel
from host_run import assert_program_compares, dump_case
from pointcloud_ref import camera_for

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_cloud as FC  # noqa: E402
import fuzz_normals as FN  # noqa: E402  (check_normals_fit: the device-against-definition comparison)

gpu = pytest.mark.gpu
RADII = (1, 2, 5, 7)
SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(FN.OUTPUTS, n)]  # every non-empty subset of the outputs


# ---- 1. the definition ------------------------------------------------------------------------------------------------
PLANE_CAM = (420.0, 390.0, 31.3, 24.6, 0.12)


def analytic_plane():
    """The plane of tests/test_pointcloud.py::test_definition_against_an_analytic_plane: n0 . P = h rendered at 48x64."""
    rows, cols = 48, 64
    fx, fy, cx, cy, B = PLANE_CAM
    n0 = np.array([0.3, -0.2, 1.0])
    n0 /= np.linalg.norm(n0)
    h = 2.0
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    a, b = B * n0[0] / h, fx * B * n0[1] / (fy * h)
    d = (a * (x - cx) + b * (y - cy) + fx * B * n0[2] / h).astype(np.float32)
    return d, n0


def angle_deg(normals, n0):
    c = np.clip(-(normals.astype(np.float64) @ n0), -1.0, 1.0)
    return np.degrees(np.arccos(c))


@pytest.mark.parametrize("radius", [2, 5, 7])
def test_definition_recovers_an_analytic_plane(radius):
    """Every pixel of the rendered plane gets a fit, borders included (their windows are cut by the image, not empty), and
    every normal is -n0 to 1e-5, the project's tolerance for its float stages."""
    d, n0 = analytic_plane()
    out = NR.disparity_normals(d, PLANE_CAM, radius, 1.0, 3)
    assert out["valid"].all() and out["normals"].dtype == np.float32
    err = np.abs(out["normals"].astype(np.float64) + n0).max()
    print("radius %d: max |normal + n0| = %.3g" % (radius, err))
    assert err <= 1e-5
    full = (2 * radius + 1) ** 2
    assert out["support"][radius:-radius, radius:-radius].min() == full and out["support"][0, 0] == (radius + 1) ** 2


def quantise_rows(d, rng):
    """Runs of 1..8 equal values along every row: each run takes the value of its first pixel."""
    q = d.copy()
    for r in range(q.shape[0]):
        k = 0
        while k < q.shape[1]:
            n = int(rng.integers(1, 9))
            q[r, k:k + n] = q[r, k]
            k += n
    return q


def test_fit_beats_central_differences_on_a_run_quantised_plane():
    """The scalar sweeps adopt a neighbour's value: a result is runs of equal disparities with steps between them.  On such
    a map central differences are zero inside a run and a spike at its edge; the plane fit at r = 5 must have less than a
    QUARTER of their median angular error over the interior pixels (a relative bound: it does not hang on one seed's degrees)."""
    d, n0 = analytic_plane()
    q = quantise_rows(d, np.random.default_rng(2024))
    assert (q != d).mean() > 0.5
    r = 5
    fit = NR.disparity_normals(q, PLANE_CAM, r, 1.0, 3)
    cd = np.zeros((3,) + q.shape, np.float32)
    cd[0, :, 1:-1] = (q[:, 2:] - q[:, :-2]) / np.float32(2)
    cd[1, 1:-1, :] = (q[2:, :] - q[:-2, :]) / np.float32(2)
    cd[2] = q
    inner = (slice(r, -r), slice(r, -r))
    e_fit = np.median(angle_deg(fit["normals"], n0)[inner])
    e_cd = np.median(angle_deg(PR.normals(cd, PLANE_CAM), n0)[inner])
    print("median angular error: fit %.3f deg, central differences %.3f deg" % (e_fit, e_cd))
    assert fit["valid"].all() and e_fit < 0.25 * e_cd


def test_edge_rules_support_and_degenerate_windows():
    cam = camera_for(9, 12)
    # a single valid row: the support is collinear, det == 0 exactly -> no fit; support 3..5 as counted at r = 2
    d = np.zeros((9, 12), np.float32)
    d[4, :] = 10.0
    out = NR.disparity_normals(d, cam, 2, 1.0, 3)
    assert not out["valid"].any() and (out["planes"] == 0).all() and (out["normals"] == 0).all()
    assert list(out["support"][4]) == [3, 4] + [5] * 8 + [4, 3] and (np.delete(out["support"], 4, axis=0) == 0).all()
    # an isolated pixel: support 1
    d = np.zeros((9, 12), np.float32)
    d[3, 7] = 25.0
    out = NR.disparity_normals(d, cam, 2, 1.0, 3)
    assert not out["valid"].any() and out["support"].sum() == 1 and out["support"][3, 7] == 1
    # n just below and at min_support: a 5x5 map at r = 1 has supports 4 (corners), 6 (edges), 9 (inside); one hole next to
    # an edge pixel takes that pixel to 5
    d = np.full((5, 5), 10.0, np.float32)
    d[1, 2] = 0.0
    out6 = NR.disparity_normals(d, camera_for(5, 5), 1, 1.0, 6)
    out5 = NR.disparity_normals(d, camera_for(5, 5), 1, 1.0, 5)
    assert out6["support"][0, 2] == 5 and out6["support"][4, 2] == 6 and out6["support"][0, 0] == 4
    assert not out6["valid"][0, 2] and out6["valid"][4, 2] and out5["valid"][0, 2] and not out5["valid"][0, 0]
    assert np.array_equal(out5["support"], out6["support"])  # the support is n, valid or not
    assert (out6["normals"][0, 2] == 0).all() and (out5["normals"][0, 2] != 0).any()


def test_edge_rules_max_diff_zero_and_step_edges():
    rng = np.random.default_rng(11)
    # max_diff = 0: only taps EQUAL to the centre count, so a = b = 0 and z = d0 bit for bit wherever there is a fit
    d = np.repeat(np.repeat(rng.uniform(5.0, 60.0, (5, 6)).astype(np.float32), 4, axis=0), 5, axis=1)  # 4x5 patches
    out = NR.fit(d, 2, 0.0, 3)
    planes, valid = out[0], out[2]
    assert valid.all() and (planes[0] == 0).all() and (planes[1] == 0).all()
    assert np.array_equal(FC.bits(planes[2]), FC.bits(d))
    # a step larger than max_diff is not smoothed across: either side's planes are those of the half-maps fitted alone
    x = np.arange(40)[None, :]
    y = np.arange(21)[:, None]
    d = (30.0 + 0.05 * x - 0.03 * y).astype(np.float32)
    d[:, 17:] += np.float32(10.0)
    d = np.concatenate([quantise_rows(d[:, :17], rng), quantise_rows(d[:, 17:], rng)], axis=1)  # no run crosses the edge
    assert np.abs(d[:, 17] - d[:, 16]).min() > 5
    for radius in (2, 5):
        whole, s_whole, _ = NR.fit(d, radius, 1.0, 3)
        left, s_left, _ = NR.fit(d[:, :17], radius, 1.0, 3)
        right, s_right, _ = NR.fit(d[:, 17:], radius, 1.0, 3)
        assert np.array_equal(FC.bits(whole[:, :, :17]), FC.bits(left)) and np.array_equal(FC.bits(whole[:, :, 17:]), FC.bits(right))
        assert np.array_equal(s_whole[:, :17], s_left) and np.array_equal(s_whole[:, 17:], s_right)
        assert (whole[2] > 0).all()


def test_edge_rules_special_values():
    cam = camera_for(9, 9)
    base = np.full((9, 9), 10.0, np.float32)
    for special, support in ((np.inf, 0), (np.nan, 0), (-0.0, 0), (0.0, 0), (-3.0, 0), (1e-45, 1), (1e-39, 1)):
        d = base.copy()
        d[4, 4] = special
        out = NR.disparity_normals(d, cam, 2, 1.0, 3)
        # the pixel itself: no tap counts for +inf (every e is NaN or -inf), one -- its own -- for a subnormal
        assert out["support"][4, 4] == support and not out["valid"][4, 4] and (out["normals"][4, 4] == 0).all(), special
        # its neighbours do not count it and keep their fit
        assert out["support"][4, 3] == 24 and out["valid"][4, 3], special
        for k in ("normals", "planes"):
            assert np.isfinite(out[k]).all(), (special, k)
    # a subnormal centre with a max_diff that spans the map: a fit, finite
    d = base.copy()
    d[4, 4] = 1e-45
    out = NR.disparity_normals(d, cam, 2, 30.0, 3)
    assert out["valid"][4, 4] and out["support"][4, 4] == 25 and np.isfinite(out["planes"]).all()
    # maps drawn with every special value: all outputs finite
    rng = np.random.default_rng(19)
    for radius, max_diff in ((1, 30.0), (2, 100.0), (5, 30.0), (7, 100.0)):  # (uniform values: few taps within 1)
        d = FC.random_disp(rng, 37, 53, valid=0.8, special=0.3)
        d.ravel()[:FC.SPECIALS.size] = FC.SPECIALS
        out = NR.disparity_normals(d, camera_for(37, 53), radius, max_diff, 3)
        assert np.isfinite(out["normals"]).all() and np.isfinite(out["planes"]).all() and out["valid"].sum() > 100
        assert not out["support"][~(d > 0)].any()
    # a max_diff near the top of binary32: only the rounding to binary32 can overflow, and the normal is still finite
    out = NR.disparity_normals(d, camera_for(37, 53), 5, 3e38, 3)
    assert np.isfinite(out["normals"]).all()


# ---- 2. the kernel's own code, run on the host ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_fit_exe(tmp_path_factory):
    """tests/cpp/normals_fit_host_main.cpp: csrc/pm_normals_fit_body.hpp compiled for the host alone, with the sanitizers."""
    return build_host_kernel(tmp_path_factory.mktemp("fithost") / "normals_fit_host_main", "normals_fit_host_main.cpp")


def _dump_case(path, disp, cam, radius, max_diff, min_support, shift):
    want = NR.disparity_normals(disp, cam, radius, max_diff, min_support)
    dump_case(path, [*disp.shape, *cam, radius, np.float32(max_diff), min_support, shift], disp=disp,
              **{"want_" + k: want[k] for k in ("normals", "planes", "support")})
    return int(want["valid"].sum())


def test_kernel_code_on_the_host_equals_the_definition(pm, host_fit_exe, tmp_path):
    """normals_fit_stage into tiles of exactly the size a workgroup's LDS tile has, then normals_fit_pixel<R> and
    normals_fit_store per pixel -- what every thread of k_normals_fit<R> runs -- over whole maps on the CPU: normals, planes
    and support equal the .npy dumps of the definition byte for byte, and AddressSanitizer / UBSan see every access.  Shapes:
    1x1, 5x3 (smaller than the window), 8x8, the odd 37x53, one pixel more than a tile either way; radii 1, 2, 5, 7."""
    tile_cols, tile_rows, per_thread = pm.normals_fit_constants()
    assert tile_cols >= 8 and tile_rows >= 1 and per_thread >= 1 and tile_cols % per_thread == 0
    rng = np.random.default_rng(41)
    fitted, k = 0, 0
    for rows, cols in ((1, 1), (5, 3), (8, 8), (37, 53), (tile_rows + 1, tile_cols + 1)):
        for radius in RADII:
            disp = FN.run_map(rng, rows, cols, valid=0.9, special=0.05) if k % 2 else FC.random_disp(rng, rows, cols, 0.8, 0.15)
            max_diff, min_support = ((1.0, 3), (30.0, 5), (0.5, 3), (1e30, 9))[k % 4]
            d = str(tmp_path / ("case%d" % k))
            fitted += _dump_case(d, disp, camera_for(rows, cols), radius, max_diff, min_support, k % 4)
            r = subprocess.run([host_fit_exe, d], capture_output=True, text=True)
            assert r.returncode == 0, ((rows, cols, radius), r.stderr[-3000:])
            k += 1
    assert fitted > 3000
    # the program does compare: one flipped bit in an expectation is a mismatch, not a pass
    assert_program_compares(host_fit_exe, d, [("want_support", np.uint8, "support differs")])


def test_headers_declare_and_the_library_exports_the_fit(pm):
    text = open(os.path.join(ROOT, "include", "pm", "imaging.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = pm.load()
    assert re.search(r"\bint\s+pm_disparity_normals\s*\(\s*pm_handle\s*\*", text)
    assert "typedef struct pm_normals_fit" in text and C.sizeof(pm.PmNormalsFit) == 12
    for name in ("pm_disparity_normals", "pm_debug_normals_fit_constants"):
        assert name in pm.EXPORTS and hasattr(lib, name), name


# ---- 3. device parity ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=48, max_cols=64) as e:
        yield e


def _shapes(pm):
    tile_cols, tile_rows, _ = pm.normals_fit_constants()
    return {"1x1": (1, 1, 0), "5x3": (5, 3, 0), "8x8": (8, 8, 0), "37x53_unaligned": (37, 53, 1),
            "tile_edges": (tile_rows + 1, 2 * tile_cols + 3, 0), "64x300": (64, 300, 0)}


@gpu
@pytest.mark.parametrize("shape", ["1x1", "5x3", "8x8", "37x53_unaligned", "tile_edges", "64x300"])
def test_fit_equals_the_definition(pm, engine, shape):
    """Radii 1, 2, 5, 7 x maps with 0, 30 % and 100 % valid pixels and 15 % special values (0, -0.0, negatives, NaN, +inf,
    subnormals) x every non-empty subset of the three outputs, plus one run-quantised map per radius; 37x53 with d_normals
    one float past a 16-byte boundary.  Bit for bit, and the bytes on either side of every output keep their pattern."""
    import torch
    rows, cols, offset = _shapes(pm)[shape]
    cam = camera_for(rows, cols)
    rng = np.random.default_rng(rows * 1000 + cols)
    fits = 0
    for radius in RADII:
        maps = [(FC.random_disp(rng, rows, cols, valid=v, special=0.15), 30.0, 3) for v in (0.0, 0.3, 1.0)]
        maps.append((FN.run_map(rng, rows, cols), 1.0, min(9, (2 * radius + 1) ** 2)))
        for disp, max_diff, min_support in maps:
            want = NR.disparity_normals(disp, cam, radius, max_diff, min_support)
            fits += int(want["valid"].sum())
            for outputs in SUBSETS:
                FN.check_normals_fit(torch, engine, disp, cam, radius, max_diff, min_support, outputs, offset, want)
    assert fits > 0 or rows * cols == 1


@gpu
def test_refused_calls_name_the_argument_and_enqueue_nothing(pm, engine):
    """Every PM_ERR_INVALID_ARG case of the header: pm_last_error names the argument, guards and payloads keep the fill."""
    import torch
    rows, cols = 16, 24
    lib, h = engine.lib, engine.h
    disp = torch.full((rows, cols), 10.0, dtype=torch.float32, device="cuda")
    outs = {k: FC.Guarded(torch, FN.WIDTH[k] * rows * cols) for k in FN.OUTPUTS}
    good = camera_for(rows, cols)

    def call(cam=good, fit=(5, 1.0, 9), d_disp=disp.data_ptr(), r=rows, c=cols, given=FN.OUTPUTS):
        cc = pm.cloud_camera(cam)
        f = pm.PmNormalsFit(*fit) if fit is not None else None
        p = lambda k: outs[k].ptr if k in given else None
        return lib.pm_disparity_normals(h, C.byref(cc) if cc is not None else None, C.byref(f) if f is not None else None, d_disp,
                                        r, c, p("normals"), p("planes"), p("support"))

    def refused(rc, word):
        text = lib.pm_last_error(h).decode()
        assert rc == pm.PM_ERR_INVALID_ARG and word in text, (rc, word, text)

    refused(call(fit=None), "fit")
    refused(call(d_disp=None), "d_disp")
    refused(call(given=()), "no output")
    refused(call(cam=None), "camera")
    for i, name in enumerate(("fx", "fy", "cx", "cy", "baseline")):
        for bad in (np.nan, np.inf, -np.inf):
            cam = list(good)
            cam[i] = bad
            refused(call(cam=cam), name)
    refused(call(cam=(0.0,) + good[1:]), "fx")
    refused(call(cam=(good[0], 0.0) + good[2:]), "fy")
    for radius in (0, -1, 8):
        refused(call(fit=(radius, 1.0, 3)), "radius")
    for max_diff in (np.nan, np.inf, -np.inf, -1.0):
        refused(call(fit=(5, max_diff, 9)), "max_diff")
    for radius, min_support in ((5, 2), (5, 0), (5, 122), (1, 10), (7, 226)):
        refused(call(fit=(radius, 1.0, min_support)), "min_support")
    for r, c in ((0, cols), (rows, 0), (-1, cols)):
        refused(call(r=r, c=c), "empty")
    engine.synchronize()
    for buf in outs.values():
        buf.read(np.uint8, 0)
    # the camera is read for d_normals alone: without that output none is needed; and the same arguments made good do run
    assert call(cam=None, given=("planes", "support")) == pm.PM_OK
    assert call(fit=(7, 0.0, 225)) == pm.PM_OK and call(fit=(1, 1.0, 9)) == pm.PM_OK
    engine.synchronize()
    assert (outs["support"].read(np.uint8).reshape(rows, cols)[1:-1, 1:-1] == 9).all()


@gpu
def test_scalar_match_to_normals_to_cloud(pm):
    """End to end on the 64x48 golden pair: a PM_MODE_SCALAR pm_match_device, pm_disparity_normals of its left map on the
    same stream, pm_point_cloud with those normals.  The organised normals equal the definition on the downloaded map, the
    compacted ones equal tests/pointcloud_ref.py on them, some normal is non-zero; a PM_MODE_PLANES handle takes the same
    call."""
    import torch
    g = np.load(os.path.join(GOLDEN, "synth64x48_cpu5.npz"))
    rows, cols = g["left"].shape
    cam = camera_for(rows, cols)
    prm = pm.default_params(int(g["sem"]), patch=int(g["patch"]), patchmatch_iters=int(g["iters"]), left_right_check=int(g["lr"]))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    L, R, SL, SR = up(g["left"]), up(g["right"]), up(g["seed_l"]), up(g["seed_r"])
    DL = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    DR = torch.zeros_like(DL)
    torch.cuda.synchronize()
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), DL.data_ptr(), DR.data_ptr())
        nrm = FC.Guarded(torch, 12 * rows * cols)
        e.disparity_normals(cam, DL.data_ptr(), rows, cols, 5, 1.0, 9, d_normals=nrm.ptr)  # ordered behind the match
        e.synchronize()
        dl = DL.cpu().numpy()
        assert np.array_equal(dl, g["disp_l"])
        got = nrm.read(np.float32).reshape(rows, cols, 3)
        want = NR.disparity_normals(dl, cam, 5, 1.0, 9)
        assert np.array_equal(FC.bits(got), FC.bits(want["normals"]))
        nonzero = (got != 0).any(axis=2)
        assert nonzero.sum() >= 1 and not nonzero[~(dl > 0)].any()
        assert np.abs(np.linalg.norm(got[nonzero].astype(np.float64), axis=1) - 1).max() <= 1e-6
        n = FC.check_cloud(torch, e, dl, cam, stride=1, normal_map=got, outputs=("xyz", "normals", "index"))
        assert n == int((dl > 0).sum()) > 0
    with pm.Engine(pm.default_params(0, patch=5, mode=pm.PM_MODE_PLANES, max_disp=24), max_rows=rows, max_cols=cols) as e:
        FN.check_normals_fit(torch, e, dl, cam, 5, 1.0, 9, want=want)  # PM_OK: the call reads a map, not the handle's state


@gpu
def test_fuzz_normals_one_short_seeded_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_normals.py"), "--cases", "40", "--seed", "3"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
