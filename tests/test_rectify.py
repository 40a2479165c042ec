"""Undistortion + rectification in front of Match() (include/pm/imaging.h: pm_rectify_u8, pm_rectify_map,
pm_match_raw_device, pm_stereo_rectify).

CPU tests pin the definition (tests/rectify_ref.py) -- hand cases, an independent interpolation, an independent
geometry (the inverse map, by iteration), the INVALID rules, a fixture the definition wrote -- and the host function
pm_stereo_rectify (loads the library, touches no device).  GPU tests hold the kernel to the definition with tolerance 0:
the geometry is binary64 with one rounding per operation in a fixed order (the build uses -ffp-contract=off, binary64
division is IEEE on the device), the interpolation is integer."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rectify_ref as RR
from conftest import GOLDEN, ROOT
from cpp_build import build_host_kernel

FIXTURE = os.path.join(GOLDEN, "rectify_37x53.npz")
DIST = (-0.28, 0.07, 2e-4, 2e-5, 0.0)  # k1, k2, p1, p2, k3


def rot(axis, deg):
    """Rotation matrix about a coordinate axis (0 = x, 1 = y, 2 = z)."""
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def radtan_view(src_rows, src_cols, rows, cols, R=None, zoom=0.7):
    """The radial-tangential view of the issue: DIST, a 2 degree rotation about y.  The raw camera sees about +-0.37 x
    +-0.26 in normalised coordinates (f = 1.35 x the source width); the new focal length is `zoom` x the raw one, scaled
    to the destination width."""
    f = 1.35 * src_cols
    cam = (f, 0.98 * f, src_cols / 2 - 0.2, src_rows / 2 + 0.4) + DIST
    fn = zoom * f * cols / src_cols
    return RR.make_view(cam, rot(1, 2.0) if R is None else R, (fn, 0.98 * fn, cols / 2 - 0.5, rows / 2 + 0.3))


def image(rows, cols, seed, n=None):
    rng = np.random.default_rng(seed)
    shape = (rows, cols) if n is None else (n, rows, cols)
    y, x = np.mgrid[0:rows, 0:cols]
    smooth = 110 + 70 * np.sin(x / 3.1) * np.cos(y / 4.3)
    return np.clip(smooth + rng.integers(-40, 41, shape), 0, 255).astype(np.uint8)


# ---- 1. the definition by hand ------------------------------------------------------------------------------------
def test_identity_view_copies_and_a_moved_principal_point_shifts_by_whole_pixels():
    src = image(23, 31, 1)
    out, valid, xy = RR.rectify(src, RR.identity_view(40.0, 40.0, 15.0, 11.0), 23, 31, border_value=77)
    assert np.array_equal(out, src) and (valid == 255).all()
    assert np.array_equal(xy[:, :, 0], np.broadcast_to(32 * np.arange(31), (23, 31)))
    assert np.array_equal(xy[:, :, 1], np.broadcast_to(32 * np.arange(23)[:, None], (23, 31)))
    # cx' + 3, cy' - 2: destination (u, v) reads source (u - 3, v + 2)
    view = RR.make_view([40.0, 40.0, 15.0, 11.0, 0, 0, 0, 0, 0], np.eye(3), [40.0, 40.0, 18.0, 9.0])
    out, valid, _ = RR.rectify(src, view, 23, 31, border_value=77)
    want = np.full((23, 31), 77, np.uint8)
    want[:21, 3:] = src[2:, :28]
    covered = np.zeros((23, 31), bool)
    covered[:21, 3:] = True
    assert np.array_equal(out, want)
    assert np.array_equal(valid, np.where(covered, 255, 0))


def test_weights_by_hand():
    """One pixel at a known fraction: ix = 32 * 1 + 8, iy = 32 * 2 + 24 -> weights 24*8, 8*8, 24*24, 8*24 over 1024."""
    src = np.arange(20, dtype=np.uint8).reshape(4, 5) * 10
    xy = np.array([[[40, 88]]], np.int32)
    out, valid = RR.remap_q5(src, xy, 0)
    total = 24 * 8 * 110 + 8 * 8 * 120 + 24 * 24 * 160 + 8 * 24 * 170
    assert out[0, 0] == (total + 512) >> 10 and valid[0, 0] == 255
    # on the last column with ax = 0 the right taps weigh nothing: still valid; with ax = 1 it is not
    out, valid = RR.remap_q5(src, np.array([[[4 * 32, 32], [4 * 32 + 1, 32]]], np.int32), 255)
    assert out[0, 0] == src[1, 4] and valid.tolist() == [[255, 0]]
    assert out[0, 1] == (31 * 32 * int(src[1, 4]) + 1 * 32 * 255 + 512) >> 10


# ---- 2. independent implementations (written apart from rectify_ref.py) ---------------------------------------------
def bilinear64(src, px, py, border):
    """float64 bilinear sample of src at (px, py), border outside."""
    H, W = src.shape
    x0, y0 = np.floor(px).astype(int), np.floor(py).astype(int)
    fx, fy = px - x0, py - y0

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(inside, src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.float64), float(border))

    top = tap(y0, x0) * (1 - fx) + tap(y0, x0 + 1) * fx
    bot = tap(y0 + 1, x0) * (1 - fx) + tap(y0 + 1, x0 + 1) * fx
    return top * (1 - fy) + bot * fy


@pytest.mark.parametrize("border", [0, 200])
def test_pixels_equal_a_float64_bilinear_sample_at_the_quantised_coordinates(border):
    """Weights are multiples of 1/32 and pixels integers: every product and sum of the float64 sample is exact, so
    floor(sample + 0.5) must equal the integer blend.  Tolerance 0."""
    src = image(41, 59, 2)
    out, _, xy = RR.rectify(src, radtan_view(41, 59, 37, 53), 37, 53, border)
    ok = xy[:, :, 0] != RR.INVALID
    assert ok.all()
    want = np.floor(bilinear64(src, xy[:, :, 0] / 32.0, xy[:, :, 1] / 32.0, border) + 0.5)
    assert np.array_equal(out.astype(np.float64), want)


def undistort(xd, yd, dist, iters=200):
    """Normalised undistorted coordinates by fixed-point iteration (converges where the distortion is mild)."""
    k1, k2, p1, p2, k3 = dist
    x, y = xd.copy(), yd.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        x, y = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / rad, (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / rad
    return x, y


def forward(view, sx, sy):
    """Raw pixel -> rectified pixel: the inverse of the map the definition evaluates."""
    cam, R, pin = view[:9], view[9:18].reshape(3, 3), view[18:]
    x, y = undistort((sx - cam[2]) / cam[0], (sy - cam[3]) / cam[1], cam[4:9])
    p = R @ np.stack([x.ravel(), y.ravel(), np.ones(x.size)])
    return (pin[0] * p[0] / p[2] + pin[2]).reshape(x.shape), (pin[1] * p[1] / p[2] + pin[3]).reshape(x.shape)


def test_the_map_inverts_to_the_destination_pixel():
    """Dequantise, undistort by iteration, rotate, project with the new pinhole: back at (u, v).  The quantisation moves
    the SOURCE position by at most 1/64 px per axis; the destination moves by that times the local magnification of the
    inverse map.  With the new focal length at most 0.7 x the raw one the magnification stays below 1 over the raw field of view
    (the radial factor's derivative 1 + 3 k1 r2 + 5 k2 r2^2 is >= 0.80 for r2 <= 0.25; 0.7 / 0.80, times 1.1 for the
    rotation's and the tangential cross terms, is 0.96): the bound is 1/64 px plus 1e-9 for the iteration."""
    rows, cols = 74, 106
    view = radtan_view(82, 118, rows, cols)
    _, valid, xy = RR.rectify(image(82, 118, 3), view, rows, cols)
    u, v = forward(view, xy[:, :, 0] / 32.0, xy[:, :, 1] / 32.0)
    vv, uu = np.mgrid[0:rows, 0:cols]
    m = valid == 255
    assert m.mean() > 0.3
    err = max(float(np.abs(u - uu)[m].max()), float(np.abs(v - vv)[m].max()))
    print("largest |destination - (u, v)| on valid pixels: %.6f px (1/64 = %.6f)" % (err, 1 / 64))
    assert err <= 1 / 64 + 1e-9


# ---- 3. INVALID ---------------------------------------------------------------------------------------------------------
def _all_invalid(out, valid, xy, border, mask):
    assert (xy[mask] == RR.INVALID).all() and (out[mask] == border).all() and (valid[mask] == 0).all()


def test_invalid_pixels():
    src = image(41, 59, 4)
    # a 100 degree rotation about y: W = R02 a + R22 = sin(100) a + cos(100) is > 0 only on the right of the image
    view = radtan_view(41, 59, 37, 53, R=rot(1, 100.0))
    out, valid, xy = RR.rectify(src, view, 37, 53, 200)
    a = (np.arange(53) - view[20]) / view[18]
    behind = np.broadcast_to(~(np.sin(np.deg2rad(100.0)) * a + np.cos(np.deg2rad(100.0)) > 0), (37, 53))
    assert 0.3 < behind.mean() < 1.0
    _all_invalid(out, valid, xy, 200, behind)
    # in front of the camera: a position, except next to the horizon W = 0, where x = X / W runs past 2^30 in Q5
    assert (xy[~behind][:, 0] != RR.INVALID).mean() > 0.5 and (np.abs(xy[~behind].astype(np.int64)) <= 2 ** 31).all()
    # a NaN entry: every pixel INVALID
    for entry in (0, 4, 9, 17, 18, 21):
        bad = radtan_view(41, 59, 37, 53)
        bad[entry] = np.nan
        out, valid, xy = RR.rectify(src, bad, 37, 53, 9)
        _all_invalid(out, valid, xy, 9, np.ones((37, 53), bool))
    # beyond 2^30 in Q5: fx = 2^27 puts |sx| * 32 past the limit wherever the distorted |x| is about 0.25 or more
    far = radtan_view(41, 59, 37, 53)
    far[0] = 2.0 ** 27
    out, valid, xy = RR.rectify(src, far, 37, 53, 31)
    inval = xy[:, :, 0] == RR.INVALID
    assert 0.05 < inval.mean() < 0.95 and (np.abs(xy[~inval].astype(np.int64)) < 2 ** 30).all()
    _all_invalid(out, valid, xy, 31, inval)
    inf = radtan_view(41, 59, 37, 53)
    inf[4] = 1e308  # k1: overflow to inf / NaN inside the polynomial
    out, valid, xy = RR.rectify(src, inf, 37, 53, 5)
    assert (xy[:, :, 0] == RR.INVALID).mean() > 0.9
    _all_invalid(out, valid, xy, 5, xy[:, :, 0] == RR.INVALID)


# ---- 4. the fixture the definition wrote ------------------------------------------------------------------------------
def test_definition_reproduces_its_fixture():
    f = np.load(FIXTURE)
    assert f["src"].shape == (41, 59) and f["out"].shape == (37, 53)
    out, valid, xy = RR.rectify(f["src"], f["view"], 37, 53, int(f["border_value"]))
    assert np.array_equal(out, f["out"]) and np.array_equal(valid, f["valid"]) and np.array_equal(xy, f["xy"])
    assert 0.02 < (f["valid"] == 0).mean() < 0.9  # the fixture has border pixels and interior pixels


# ---- 5. pm_stereo_rectify (host only) -----------------------------------------------------------------------------------
CAM1 = (458.654, 457.296, 367.215, 248.375) + DIST
CAM2 = (457.587, 456.134, 379.999, 255.238, -0.283, 0.074, -1.0e-4, -3.5e-5, 0.0)
R_REL = rot(2, 2.0) @ rot(1, 3.0) @ rot(0, 5.0)
T_REL = np.array([-0.11, 0.004, -0.002])


def test_stereo_rectify_rotations_and_baseline(pm):
    v1, v2, base = pm.stereo_rectify(CAM1, CAM2, R_REL, T_REL)
    for v in (v1, v2):
        R = v[9:18].reshape(3, 3)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1) <= 1e-12
    t = v2[9:18].reshape(3, 3) @ T_REL
    n = float(np.sqrt(T_REL[0] * T_REL[0] + T_REL[1] * T_REL[1] + T_REL[2] * T_REL[2]))
    assert t[0] < 0 and abs(t[1]) <= 1e-12 * n and abs(t[2]) <= 1e-12 * n
    assert abs(base - n) <= 1e-15
    # the relative rotation that is left between the rectified cameras is the identity: R2 R R1^T = I
    assert np.abs(v2[9:18].reshape(3, 3) @ R_REL @ v1[9:18].reshape(3, 3).T - np.eye(3)).max() <= 1e-12
    # the cameras come back untouched; the common pinhole
    assert np.array_equal(v1[:9], np.array(CAM1)) and np.array_equal(v2[:9], np.array(CAM2))
    f = min(CAM1[1], CAM2[1])
    pin = [f, f, (CAM1[2] + CAM2[2]) / 2, (CAM1[3] + CAM2[3]) / 2]
    assert np.array_equal(v1[18:], pin) and np.array_equal(v2[18:], pin)


def test_stereo_rectify_identity_case_is_exact(pm):
    v1, v2, base = pm.stereo_rectify(CAM1, CAM2, np.eye(3), [-0.12, 0.0, 0.0])
    assert np.array_equal(v1[9:18], np.eye(3).ravel()) and np.array_equal(v2[9:18], np.eye(3).ravel())
    assert abs(base - 0.12) <= 1e-15


def test_stereo_rectify_refuses_what_it_cannot_rectify(pm):
    for R, T in ((np.eye(3), [0.0, 0.0, 0.0]), (np.eye(3), [0.11, 0.0, 0.0]), (rot(1, 179.0), T_REL),
                 (np.eye(3), [np.nan, 0.0, 0.0]), (np.full((3, 3), np.inf), T_REL)):
        with pytest.raises(pm.PmError) as err:
            pm.stereo_rectify(CAM1, CAM2, R, T)
        assert err.value.status == pm.PM_ERR_INVALID_ARG
    bad = list(CAM1)
    bad[4] = np.nan
    with pytest.raises(pm.PmError):
        pm.stereo_rectify(bad, CAM2, R_REL, T_REL)
    import ctypes as C
    lib = pm.load()
    assert lib.pm_stereo_rectify(None, None, None, None, None, None, None) == pm.PM_ERR_INVALID_ARG
    v = pm.PmRectifyView()
    assert lib.pm_stereo_rectify(None, None, None, None, C.byref(v), C.byref(v), None) == pm.PM_ERR_INVALID_ARG


def project_raw(cam, X):
    """3-D points (N, 3) in a raw camera's frame -> its distorted pixels."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam
    x, y = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
    r2 = x * x + y * y
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    return (fx * (x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + cx,
            fy * (y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + cy)


def test_stereo_rectify_puts_points_on_equal_rows_with_the_pinhole_disparity(pm):
    v1, v2, base = pm.stereo_rectify(CAM1, CAM2, R_REL, T_REL)
    rng = np.random.default_rng(7)
    X1 = np.stack([rng.uniform(-0.8, 0.8, 200), rng.uniform(-0.5, 0.5, 200), rng.uniform(1.5, 6.0, 200)], axis=1)
    X2 = X1 @ R_REL.T + T_REL
    assert (X2[:, 2] > 1.0).all()
    u1, r1 = forward(v1, *project_raw(CAM1, X1))
    u2, r2 = forward(v2, *project_raw(CAM2, X2))
    Z = (X1 @ v1[9:18].reshape(3, 3).T)[:, 2]
    assert np.abs(Z - (X2 @ v2[9:18].reshape(3, 3).T)[:, 2]).max() <= 1e-12
    row_err = float(np.abs(r1 - r2).max())
    disp_err = float(np.abs((u1 - u2) - v1[18] * base / Z).max())
    print("rows differ by at most %.3e px, disparity from f B / Z by at most %.3e px" % (row_err, disp_err))
    assert row_err <= 1e-9 and disp_err <= 1e-9 and (u1 - u2 > 0).all()


# ---- 6. the kernel's own per-thread code, run on the host --------------------------------------------------------------
@pytest.fixture(scope="module")
def host_kernel_exe(tmp_path_factory):
    """tests/cpp/rectify_host_main.cpp: csrc/pm_rectify.hpp compiled for the host alone, with the sanitizers."""
    return build_host_kernel(tmp_path_factory.mktemp("rectifyhost") / "rectify_host_main", "rectify_host_main.cpp")


def test_kernel_code_on_the_host_equals_the_definition(host_kernel_exe, tmp_path):
    """rectify_four<Gray> and <Map> -- what every thread of k_rectify runs -- over whole images on the CPU: pixels, mask and
    map equal the definition with tolerance 0, nothing is written outside the images, and AddressSanitizer / UBSan see
    every access.  Random cases from the fuzzer's generator (sizes <= 48x64) plus the odd strided case of the device tests."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fuzz_rectify import random_view
    rng = np.random.default_rng(21)
    cases = [(3, 41, 59, 64, 37, 53, 200, 1, 1, radtan_view(41, 59, 37, 53)),
             (1, 41, 59, 64, 37, 53, 0, 0, 1, radtan_view(41, 59, 37, 53, R=rot(1, 100.0))),
             (1, 3, 3, 3, 8, 5, 200, 0, 0, radtan_view(3, 3, 8, 5))]
    for _ in range(40):
        sr, sc, rows, cols = (int(rng.integers(1, 49)), int(rng.integers(1, 65)), int(rng.integers(1, 49)),
                              int(rng.integers(1, 65)))
        cases.append((int(rng.choice([1, 2, 3])), sr, sc, sc + int(rng.choice([0, 1, 5])), rows, cols, int(rng.integers(0, 256)),
                      int(rng.integers(0, 4)), int(rng.integers(0, 2)), random_view(rng, sr, sc, rows, cols)[1]))
    raws = []
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for n, sr, sc, step, rows, cols, border, shift, mask, view in cases:
            raws.append(rng.integers(0, 256, (n, sr, step), dtype=np.uint8))
            f.write(np.array([n, sr, sc, step, rows, cols, border, shift, mask], np.int32).tobytes())
            f.write(np.asarray(view, np.float64).tobytes())
            f.write(raws[-1].tobytes())
    r = subprocess.run([host_kernel_exe, "gray", str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    buf, pos = np.fromfile(tmp_path / "out.bin", np.uint8), 0
    for (n, sr, sc, step, rows, cols, border, shift, mask, view), raw in zip(cases, raws):
        total = n * rows * cols
        dst, val = buf[pos:pos + total + 8], buf[pos + total + 8:pos + 2 * (total + 8)]
        pos += 2 * (total + 8)
        xy = buf[pos:pos + rows * cols * 8].view(np.int32).reshape(rows, cols, 2)
        pos += rows * cols * 8
        want, want_valid, want_xy = RR.rectify(raw[:, :, :sc], view, rows, cols, border)
        what = (n, sr, sc, step, rows, cols, border, shift, mask)
        assert np.array_equal(dst[shift:shift + total].reshape(want.shape), want), what
        assert (dst[:shift] == 0xA5).all() and (dst[shift + total:] == 0xA5).all(), what
        assert np.array_equal(xy, want_xy), what
        if mask:
            assert np.array_equal(val[shift:shift + total].reshape(want.shape), want_valid), what
            assert (val[:shift] == 0xA5).all() and (val[shift + total:] == 0xA5).all(), what
        else:
            assert (val == 0xA5).all(), what
    assert pos == buf.size


# ---- device parity ------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        yield e


def _view(kind, src_rows, src_cols, rows, cols):
    if kind == "identity":
        return RR.identity_view(1.2 * src_cols, 1.2 * src_cols, src_cols / 2, src_rows / 2)
    if kind == "behind":
        return radtan_view(src_rows, src_cols, rows, cols, R=rot(1, 100.0))
    return radtan_view(src_rows, src_cols, rows, cols)


# name: src rows, src cols, src_step, rows, cols, n, border, view, dst offset, caller stream
DEVICE_CASES = {
    "odd_strided": (41, 59, 64, 37, 53, 1, 0, "radtan", 0, False),
    "odd_strided_n3_border200": (41, 59, 64, 37, 53, 3, 200, "radtan", 0, False),
    "odd_identity": (41, 59, 64, 37, 53, 1, 200, "identity", 0, False),
    "odd_behind": (41, 59, 64, 37, 53, 1, 200, "behind", 0, False),
    "64x96": (64, 96, 0, 64, 96, 1, 0, "radtan", 0, False),
    "64x96_identity_border200": (64, 96, 0, 64, 96, 1, 200, "identity", 0, False),
    "64x96_behind_n3": (64, 96, 0, 64, 96, 3, 0, "behind", 0, False),
    "tiny_all_border": (3, 3, 0, 8, 5, 1, 200, "radtan", 0, False),
    "tiny_all_border_0": (3, 3, 0, 8, 5, 3, 0, "identity", 0, False),
    "unaligned_dst": (64, 96, 0, 64, 96, 1, 0, "radtan", 1, False),
    "unaligned_dst_odd_n3": (41, 59, 64, 37, 53, 3, 200, "radtan", 1, False),
    "caller_stream": (64, 96, 0, 64, 96, 3, 200, "radtan", 0, True),
    "caller_stream_odd": (41, 59, 64, 37, 53, 1, 0, "radtan", 0, True),
}
_wanted = {}


def _case(name):
    """Inputs and the definition's outputs of a device case, computed once."""
    if name not in _wanted:
        sr, sc, step, rows, cols, n, border, kind, _, _ = DEVICE_CASES[name]
        pitch = step if step else sc
        raw = np.random.default_rng(sr * 7 + cols).integers(0, 256, (n, sr, pitch), dtype=np.uint8)
        raw[:, :, :sc] = image(sr, sc, cols + n, n)
        view = _view(kind, sr, sc, rows, cols)
        _wanted[name] = (raw, view) + RR.rectify(raw[:, :, :sc], view, rows, cols, border)
    return _wanted[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DEVICE_CASES))
def test_device_pixels_mask_and_map_equal_the_definition(engine, name):
    import torch
    sr, sc, step, rows, cols, n, border, kind, offset, own_stream = DEVICE_CASES[name]
    raw, view, want, want_valid, want_xy = _case(name)
    if kind == "radtan" and sr > 8:
        assert 0 < (want_valid == 0).mean() < 0.9  # border and interior both present
    total = n * rows * cols
    d_src = _dev(raw)
    d_dst = torch.full((total + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    d_val = torch.full((total + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    d_xy = torch.zeros((rows, cols, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream() if own_stream else None
    engine.rectify_u8(view, d_src.data_ptr(), n, sr, sc, step, rows, cols, border, d_dst.data_ptr() + offset,
                      d_val.data_ptr() + offset, side.cuda_stream if side else None)
    engine.rectify_map(view, rows, cols, d_xy.data_ptr())
    if side:
        side.synchronize()
    engine.synchronize()
    got, got_valid = d_dst.cpu().numpy(), d_val.cpu().numpy()
    for g, w, what in ((got, want, "pixels"), (got_valid, want_valid, "mask")):
        inner = g[offset:offset + total].reshape(w.shape)
        assert np.array_equal(inner, w), "%s: %d of %d differ" % (what, int((inner != w).sum()), w.size)
        assert (g[:offset] == 0xA5).all() and (g[offset + total:] == 0xA5).all(), what + ": written outside the image"
    assert np.array_equal(d_xy.cpu().numpy(), want_xy)
    # without a mask the pixels are the same
    d_dst.fill_(0xA5)
    torch.cuda.synchronize()
    engine.rectify_u8(view, d_src.data_ptr(), n, sr, sc, step, rows, cols, border, d_dst.data_ptr() + offset, None, None)
    engine.synchronize()
    assert np.array_equal(d_dst.cpu().numpy()[offset:offset + total].reshape(want.shape), want)


@pytest.mark.gpu
def test_device_reproduces_the_fixture(engine):
    import torch
    f = np.load(FIXTURE)
    d_src = _dev(f["src"])
    d_dst = torch.empty((37, 53), dtype=torch.uint8, device="cuda")
    engine.rectify_u8(f["view"], d_src.data_ptr(), 1, 41, 59, 0, 37, 53, int(f["border_value"]), d_dst.data_ptr())
    engine.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), f["out"])


def _match_pair(synth):
    p = synth.make_pair(5, rows=64, cols=96, n_points=30, dilate_factor=2)
    vl = radtan_view(64, 96, 64, 96, zoom=1.0)
    vr = radtan_view(64, 96, 64, 96, R=rot(0, 0.7) @ rot(1, -1.5), zoom=1.0)
    return p, vl, vr


MATCH_MODES = {
    "scalar_cpu_semantics": dict(sem=0, kw=dict(patch=5, patchmatch_iters=2), seeded=True),
    "planes_f32": dict(sem=0, kw=dict(patch=5, patchmatch_iters=2, mode=1, state_dtype=0, max_disp=32), seeded=True),
    # max_disp 40: with the default 128 the seeder's search stripe is wider than a 96-pixel image and it finds no seed
    "self_seeded": dict(sem=1, kw=dict(patch=5, patchmatch_iters=2, sparse_init=1, max_disp=40), seeded=False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MATCH_MODES))
def test_match_raw_equals_rectify_then_match(pm, synth, mode):
    import torch
    assert pm.PM_SEM_CPU == 0 and pm.PM_MODE_PLANES == 1  # the numbers MATCH_MODES uses
    m = MATCH_MODES[mode]
    rows, cols = 64, 96
    p, vl, vr = _match_pair(synth)
    with pm.Engine(pm.default_params(m["sem"], **m["kw"]), max_rows=rows, max_cols=cols) as e:
        L, R = _dev(p["left"]), _dev(p["right"])
        SL, SR = _dev(p["seed_l"]), _dev(p["seed_r"])
        sl, sr = (SL.data_ptr(), SR.data_ptr()) if m["seeded"] else (None, None)
        RL, RRt = torch.empty_like(L), torch.empty_like(R)
        out = [torch.full((rows, cols), -7.0, device="cuda") for _ in range(6)]
        torch.cuda.synchronize()
        e.rectify_u8(vl, L.data_ptr(), 1, rows, cols, 0, rows, cols, 0, RL.data_ptr())
        e.rectify_u8(vr, R.data_ptr(), 1, rows, cols, 0, rows, cols, 0, RRt.data_ptr())
        e.match_device(1, RL.data_ptr(), RRt.data_ptr(), rows, cols, sl, sr, out[0].data_ptr(), out[1].data_ptr())
        e.match_raw_device(1, vl, vr, L.data_ptr(), R.data_ptr(), rows, cols, 0, rows, cols, sl, sr, out[2].data_ptr(),
                           out[3].data_ptr())
        e.match_raw_device(1, vl, vr, L.data_ptr(), R.data_ptr(), rows, cols, 0, rows, cols, sl, sr, out[4].data_ptr(),
                           out[5].data_ptr())  # again: the scratch is reused
        e.synchronize()
        got = [t.cpu().numpy() for t in out]
        assert np.array_equal(RL.cpu().numpy(), RR.rectify(p["left"], vl, rows, cols)[0])
    assert not (got[0] == -7.0).all() and len(np.unique(got[0])) > 10
    for k in (2, 4):
        assert np.array_equal(got[k], got[0]) and np.array_equal(got[k + 1], got[1])


@pytest.mark.gpu
def test_match_raw_with_identity_views_equals_match_device(pm, synth):
    import torch
    rows, cols = 64, 96
    p = synth.make_pair(5, rows=rows, cols=cols, n_points=30, dilate_factor=2)
    ident = RR.identity_view(100.0, 100.0, 48.0, 32.0)
    with pm.Engine(pm.default_params(0, patch=5, patchmatch_iters=2), max_rows=rows, max_cols=cols) as e:
        L, R = _dev(p["left"]), _dev(p["right"])
        SL, SR = _dev(p["seed_l"]), _dev(p["seed_r"])
        out = [torch.empty((rows, cols), device="cuda") for _ in range(4)]
        e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), out[0].data_ptr(),
                       out[1].data_ptr())
        e.match_raw_device(1, ident, ident, L.data_ptr(), R.data_ptr(), rows, cols, 0, rows, cols, SL.data_ptr(),
                           SR.data_ptr(), out[2].data_ptr(), out[3].data_ptr())
        e.synchronize()
        got = [t.cpu().numpy() for t in out]
    assert np.array_equal(got[2], got[0]) and np.array_equal(got[3], got[1])


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing(pm, engine):
    import torch
    sr, sc, rows, cols = 41, 59, 37, 53
    view = radtan_view(sr, sc, rows, cols)
    d_src = _dev(image(sr, sc, 8))
    d_dst = torch.full((rows * cols,), 0x5A, dtype=torch.uint8, device="cuda")
    d_val = torch.full((rows * cols,), 0x5A, dtype=torch.uint8, device="cuda")
    d_xy = torch.full((rows, cols, 2), 0x5A5A, dtype=torch.int32, device="cuda")
    d_disp = torch.full((2, rows, cols), -7.0, device="cuda")
    torch.cuda.synchronize()

    def changed(entry, value):
        v = view.copy()
        v[entry] = value
        return v

    ok = dict(view=view, d_src=d_src.data_ptr(), n=1, src_rows=sr, src_cols=sc, src_step=0, rows=rows, cols=cols,
              border_value=0, d_dst=d_dst.data_ptr(), d_valid=d_val.data_ptr())
    bad_views = [None] + [changed(i, x) for i in (0, 5, 9, 17, 18, 21) for x in (np.nan, np.inf, -np.inf)] + \
                [changed(18, 0.0), changed(19, 0.0), changed(19, -0.0)]
    bad = [dict(view=v) for v in bad_views] + [dict(d_src=None), dict(d_dst=None), dict(rows=0), dict(cols=0),
                                               dict(rows=-3), dict(cols=-1), dict(border_value=-1),
                                               dict(border_value=256), dict(n=0), dict(src_rows=0), dict(src_cols=0),
                                               dict(src_step=sc - 1)]
    for change in bad:
        with pytest.raises(pm.PmError) as err:
            engine.rectify_u8(**dict(ok, **change))
        assert err.value.status == pm.PM_ERR_INVALID_ARG and "pm_rectify_u8" in str(err.value), change
    for kw in [dict(view=v) for v in bad_views] + [dict(d_xy=None), dict(rows=0), dict(cols=0)]:
        with pytest.raises(pm.PmError) as err:
            engine.rectify_map(**dict(dict(view=view, rows=rows, cols=cols, d_xy=d_xy.data_ptr()), **kw))
        assert err.value.status == pm.PM_ERR_INVALID_ARG, kw
    raw_ok = dict(n=1, left_view=view, right_view=view, d_left_raw=d_src.data_ptr(), d_right_raw=d_src.data_ptr(),
                  src_rows=sr, src_cols=sc, src_step=0, rows=rows, cols=cols, d_seed_l=None, d_seed_r=None,
                  d_disp_l=d_disp[0].data_ptr(), d_disp_r=d_disp[1].data_ptr())
    raw_bad = [(dict(left_view=None), pm.PM_ERR_INVALID_ARG), (dict(right_view=changed(3, np.nan)), pm.PM_ERR_INVALID_ARG),
               (dict(left_view=changed(18, 0.0)), pm.PM_ERR_INVALID_ARG), (dict(d_left_raw=None), pm.PM_ERR_INVALID_ARG),
               (dict(d_right_raw=None), pm.PM_ERR_INVALID_ARG), (dict(d_disp_l=None), pm.PM_ERR_INVALID_ARG),
               (dict(rows=0), pm.PM_ERR_INVALID_ARG), (dict(cols=0), pm.PM_ERR_INVALID_ARG),
               (dict(rows=65), pm.PM_ERR_SIZE), (dict(cols=97), pm.PM_ERR_SIZE), (dict(rows=4000, cols=4000), pm.PM_ERR_SIZE)]
    for change, status in raw_bad:
        with pytest.raises(pm.PmError) as err:
            engine.match_raw_device(**dict(raw_ok, **change))
        assert err.value.status == status, change
    engine.synchronize()
    assert (d_dst.cpu().numpy() == 0x5A).all() and (d_val.cpu().numpy() == 0x5A).all()
    assert (d_xy.cpu().numpy() == 0x5A5A).all() and (d_disp.cpu().numpy() == -7.0).all()
    # the handle is still usable
    engine.rectify_u8(**ok)
    engine.synchronize()
    assert np.array_equal(d_dst.cpu().numpy().reshape(rows, cols), RR.rectify(image(sr, sc, 8), view, rows, cols)[0])


@pytest.mark.gpu
def test_differential_fuzz_of_the_rectification():
    """tools/fuzz_rectify.py: random sizes, strides, image counts, borders, alignments, streams and views (mild to absurd
    distortion, rotations past 90 degrees), pixels / mask / map == tests/rectify_ref.py bit for bit."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_rectify.py"), "--cases", "20", "--seed", "11",
                        "--max-rows", "96", "--max-cols", "128"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
