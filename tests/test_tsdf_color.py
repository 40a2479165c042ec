"""Colour in the TSDF model: a colour volume beside the distance volume, integrated with it and gathered back
(include/pm/imaging.h: pm_tsdf_color_bytes, pm_tsdf_color_clear, pm_tsdf_integrate_color, pm_tsdf_color_map, pm_tsdf_color_points).

CPU tests pin the definition (tests/tsdf_color_ref.py) on the analytic plane-and-box scene of tests/test_tsdf.py, painted with a
texture that is an analytic function of the world position -- constant colour, the band, weights and special values, the sampler's
edges -- and show ON THE DEFINITION ALONE that six noisy images fused into the volume give a better colour than one noisy image,
and that the mesh of the fused model is coloured.  The kernels' own per-thread code (csrc/pm_tsdf_color_body.hpp) runs on the host
under ASan / UBSan, spans and blocks forwards and backwards.  GPU tests hold the kernels to the definition with tolerance 0 and
guard bands around every buffer."""
import copy
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tsdf_color_ref as CR
import tsdf_mesh_ref as MR
import tsdf_ref as TR
from conftest import ROOT
from cpp_build import build_host_kernel
from host_run import assert_program_compares, dump_case
from test_reproject import CAM
from test_stage_refusal_order import (BAD_VOLUME, NAN, both, c_camera, c_motion_ref, c_struct, c_volume, camera_steps, fix,
                                      motion_steps, shape_steps, size_step, tsdf_common_steps, volume_steps, walk)
from test_tsdf import (ARC, BOX, COLS, GRID, IDENT, MAPS, ROWS, VOLUMES, Z0, case_camera, case_grid, case_map, case_pose, fused_model,
                       one_view, render)

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_tsdf as FT  # noqa: E402  (Guarded, bits, WEIGHT_SPECIALS, random_weight)

gpu = pytest.mark.gpu
bits = FT.bits


# ---- the painted scene ---------------------------------------------------------------------------------------------------------
def texture(P):
    """The scene's colour (b, g, r in levels of 0 .. 255, binary64) as an analytic function of the world position."""
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    return np.stack([128 + 60 * np.sin(6 * x + 1), 128 + 60 * np.cos(5 * y), 90 + 400 * (Z0 - z)], -1)


def world_points(pose, disp, cam=CAM):
    """The world position each pixel of a left map at `pose` sees (binary64; the camera's centre where it has no value)."""
    rows, cols = disp.shape
    fx, fy, cx, cy, baseline = cam
    R = np.asarray(pose[0], np.float64).reshape(3, 3)
    c = -(R.T @ np.asarray(pose[1], np.float64))
    x, y = np.arange(cols)[None, :], np.arange(rows)[:, None]
    d = np.stack(np.broadcast_arrays((x - cx) / fx, (y - cy) / fy, np.ones((rows, cols))), -1) @ R
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(disp > 0, fx * baseline / disp.astype(np.float64), 0.0)
    return c + s[..., None] * d


def paint(pose, disp, rng=None, noise=0.0):
    """The float image of the scene at `pose`: the texture where the noiseless map has a value, +0.0 elsewhere."""
    img = texture(world_points(pose, disp))
    if rng is not None:
        img = img + rng.uniform(-noise, noise, img.shape)
    return np.where((disp > 0)[..., None], img, 0.0).astype(np.float32)


def integrate(colors, disp, image, pose=IDENT, voxels=None, grid=GRID, **kw):
    """CR.integrate on the scene's grid; asserts what holds in every case: the distance volume and counts [0], [1] are
    tsdf_ref.integrate's, bit for bit."""
    voxels = TR.clear(grid) if voxels is None else voxels
    out = CR.integrate(grid, voxels, colors, disp, image, CAM, *pose, **kw)
    plain = TR.integrate(grid, voxels, disp, CAM, *pose, **{k: v for k, v in kw.items() if k != "band"})
    assert np.array_equal(bits(out["voxels"]), bits(plain["voxels"])) and tuple(out["counts"][:2]) == tuple(plain["counts"])
    assert out["counts"][2] == out["colored"].sum() and not (out["colored"] & ~out["updated"]).any()
    return out


# ---- 1. the definition ----------------------------------------------------------------------------------------------------
BYTES = np.array([17, 130, 251], np.uint8)


def test_definition_a_constant_colour_is_stored_and_returned_exactly():
    """A constant byte image with unit weights: every coloured voxel holds exactly those bytes as floats ((0 * 0 + p * 1) / 1), and
    pm_tsdf_color_map of the model's render at the same pose, with byte_scale 1, returns exactly those bytes at every coloured
    pixel: the normalised mean of equal values may leave the value by a rounding or two, never by half a level."""
    truth, _ = one_view()
    image = np.broadcast_to(BYTES, (ROWS, COLS, 3)).copy()
    out = integrate(CR.clear(GRID), truth, image)
    col = out["colored"]
    assert col.sum() > 10000 and col.sum() == out["counts"][1] - (np.abs(out["sdf"][out["updated"]]) > GRID["trunc"]).sum()
    assert (out["colors"][col] == np.array([17, 130, 251, 1], np.float32)).all() and (bits(out["colors"][~col]) == 0).all()
    ray = TR.raycast(GRID, out["voxels"], CAM, *IDENT, ROWS, COLS, min_range=1.2, max_range=2.4, step=0.5, min_weight=0.0)
    for disp in (ray["disp"], truth):
        got = CR.color_map(GRID, out["colors"], disp, CAM, *IDENT, byte_scale=1.0)
        m = got["colored"]
        assert m.sum() == got["counts"][0] >= 0.9 * (disp > 0).sum() and not (m & ~(disp > 0)).any()
        assert (got["bgr8"][m] == BYTES).all() and np.abs(got["bgr"][m] - BYTES.astype(np.float32)).max() < 1e-4
        assert (got["bgr8"][~m] == 0).all() and (bits(got["bgr"][~m]) == 0).all()
    twice = CR.color_map(GRID, out["colors"], truth, CAM, *IDENT, byte_scale=2.0)
    assert (twice["bgr8"][twice["colored"]] == np.array([34, 255, 255], np.uint8)).all()  # saturated


def test_definition_the_band_decides_and_the_rest_keeps_poisoned_records():
    """band < 1: exactly the updated voxels whose sdf lies within band * trunc are coloured -- counted here from the definition's
    own sdf -- and every other record keeps its bits, NaN payloads included."""
    truth, _ = one_view()
    image = paint(IDENT, truth)
    poison = np.full((GRID["nz"], GRID["ny"], GRID["nx"], 4), np.nan, np.float32)
    poison.view(np.uint32)[...] = (0x7FC00001, 0xFFC00000, 0x7F800123, 0xFFFFFFFF)
    counts = []
    for band in (0.25, 0.5, 1.0):
        out = integrate(poison, truth, image, band=band)
        bandw = np.float64(np.float32(band)) * GRID["trunc"]
        want = out["updated"] & (np.abs(out["sdf"]) <= bandw)
        assert np.array_equal(out["colored"], want) and 0 < want.sum() < out["updated"].sum()
        assert np.array_equal(bits(out["colors"][~want]), bits(poison[~want]))
        counts.append(int(want.sum()))
    print("coloured at band 0.25, 0.5, 1:", counts)
    assert counts[0] < counts[1] < counts[2]
    # the band is closed: a voxel exactly on it is coloured (sdf = 0.03 = 0.5 * 0.06 does not occur by chance; the rule is <=)
    assert np.float64(np.float32(0.5)) * 0.06 == 0.03


def test_definition_a_second_integrate_keeps_the_colour_and_raises_the_weight():
    truth, _ = one_view()
    image = np.random.default_rng(5).integers(0, 256, (ROWS, COLS, 3)).astype(np.uint8)
    for max_weight, want_w in ((64.0, (2.0, 3.0)), (2.0, (2.0, 2.0)), (1.5, (1.5, 1.5))):
        grid = dict(GRID, max_weight=max_weight)
        first = integrate(CR.clear(grid), truth, image, grid=grid, band=0.5)
        col = first["colored"]
        second = integrate(first["colors"], truth, image, voxels=first["voxels"], grid=grid, band=0.5)
        assert np.array_equal(second["colored"], col)
        # ((p * 1) + (p * 1)) / 2 is p for a byte p; with w = 1.5: ((p * 1.5) + p) / 2.5 is exact too (small integers, times 5 / 2)
        assert np.array_equal(bits(second["colors"][..., :3]), bits(first["colors"][..., :3]))
        assert (second["colors"][..., 3][col] == np.float32(want_w[0])).all() and (second["colors"][..., 3][~col] == 0).all()
        third = integrate(second["colors"], truth, image, voxels=second["voxels"], grid=grid, band=0.5)
        assert (third["colors"][..., 3][col] == np.float32(want_w[1])).all()
        assert np.abs(third["colors"][..., :3] - first["colors"][..., :3]).max() <= 2.0 ** -16


def test_definition_every_special_weight_and_pixel():
    """pm_tsdf_integrate's weight rule decides the colour as it decides the distance; a float pixel with a NaN or an infinity in
    any channel leaves the colour alone while the distance is still updated."""
    truth, plain = one_view()
    w = np.ones((ROWS, COLS), np.float32)
    w[:, :9 * 8] = np.repeat(FT.WEIGHT_SPECIALS, 8)[None, :]
    takes = np.isfinite(w) & (w > 0)
    image = paint(IDENT, truth)
    ref = integrate(CR.clear(GRID), truth, image)
    out = integrate(CR.clear(GRID), truth, image, weight=w)
    X, Y, Z = TR.voxel_centres(GRID)
    _, iu, iv, _ = TR.project(X, Y, Z, CAM, *IDENT, ROWS, COLS)
    iu, iv = np.broadcast_to(iu, ref["colored"].shape), np.broadcast_to(iv, ref["colored"].shape)
    assert np.array_equal(out["colored"], ref["colored"] & takes[iv, iu]) and 0 < out["counts"][2] < ref["counts"][2]
    col = out["colored"]
    assert np.array_equal(bits(out["colors"][..., 3][col]), bits(w[iv, iu][col]))  # min(0 + wn, 64)
    exact = col & np.isin(w[iv, iu], (0.25, 1.0))
    # ((0 * 0) + (p * wn)) / wn is p where wn is a power of two
    assert exact.sum() > 500 and np.array_equal(bits(out["colors"][..., :3][exact]), bits(ref["colors"][..., :3][exact]))
    bad = image.copy()
    specials = np.array([np.nan, np.inf, -np.inf], np.float32)
    for k in range(9):  # channel k % 3 of the pixels of columns 8k .. 8k + 7 holds special k // 3
        bad[:, 8 * k:8 * k + 8, k % 3] = specials[k // 3]
    spoiled = ~np.isfinite(bad).all(-1)
    out = integrate(CR.clear(GRID), truth, bad)
    assert np.array_equal(out["colored"], ref["colored"] & ~spoiled[iv, iu]) and (ref["colored"] & spoiled[iv, iu]).sum() > 500
    assert np.array_equal(out["updated"], plain["updated"]) and np.isfinite(out["colors"]).all()
    as_bytes = integrate(CR.clear(GRID), truth, np.clip(np.rint(image), 0, 255).astype(np.uint8))
    assert np.array_equal(as_bytes["colored"], ref["colored"])  # a byte image has no special values


# ---- 2. fusion: on the definition alone -----------------------------------------------------------------------------------------
NOISE, BAND = 20.0, 0.5


@functools.lru_cache(maxsize=None)
def fused_colour():
    """test_tsdf.fused_model's six noisy maps, each with the scene's texture under U(-20, 20) levels of independent noise,
    integrated in turn with band 0.5 (three voxels either side of the surface)."""
    vol, maps, _, _, ray = fused_model()
    rng = np.random.default_rng(11)
    v, col = TR.clear(GRID), CR.clear(GRID)
    for pose, d in zip(ARC[:6], maps):
        out = CR.integrate(GRID, v, col, d, paint(pose, render(pose), rng, NOISE), CAM, *pose, band=BAND)
        v, col = out["voxels"], out["colors"]
    assert np.array_equal(bits(v), bits(vol))
    return v, col, ray, rng


def test_conditions_the_fused_colour_beats_a_single_noisy_image():
    """Read back at the seventh pose, off the arc, through pm_tsdf_raycast's render: against the noiseless texture at the hit
    points the RMS error of the fused colour is SMALLER than that of one noisy image at that pose, and at least half of the hit
    pixels are coloured.  Reached: 3.16 against 11.49 levels, 3454 of 3455 hit pixels coloured."""
    _, col, ray, rng = fused_colour()
    got = CR.color_map(GRID, col, ray["disp"], CAM, *ARC[6])
    want = texture(world_points(ARC[6], ray["disp"]))
    one = want + np.random.default_rng(12).uniform(-NOISE, NOISE, want.shape)
    m = got["colored"]
    rms = lambda a: float(np.sqrt(np.mean((a[m] - want[m]) ** 2)))
    print("hit %d, coloured %d, RMS fused %.3f, one noisy image %.3f levels" % (ray["hit"].sum(), m.sum(), rms(got["bgr"].astype(np.float64)), rms(one)))
    assert not (m & ~ray["hit"]).any() and m.sum() >= 0.5 * ray["hit"].sum()
    assert rms(got["bgr"].astype(np.float64)) < rms(one)


def test_conditions_the_mesh_of_the_fused_model_is_coloured():
    """tsdf_mesh_ref's vertices of the fused model through pm_tsdf_color_points: EVERY vertex on the observed surface -- within a
    voxel of the plane or of the box's front face, two voxels away from the box's outline -- is coloured.  Of all vertices, the
    spurious sheets along the box's occlusion boundary included, 98 % are (6834 of 6973)."""
    v, col, _, _ = fused_colour()
    mesh = MR.mesh(GRID, v)
    got = CR.color_points(GRID, col, mesh["xyz"], byte_scale=1.0)
    P = mesh["xyz"].astype(np.float64)
    inside = (P[:, 0] > BOX[0][0] + .01) & (P[:, 0] < BOX[0][1] - .01) & (P[:, 1] > BOX[1][0] + .01) & (P[:, 1] < BOX[1][1] - .01)
    outside = (P[:, 0] < BOX[0][0] - .02) | (P[:, 0] > BOX[0][1] + .02) | (P[:, 1] < BOX[1][0] - .02) | (P[:, 1] > BOX[1][1] + .02)
    on = (inside & (np.abs(P[:, 2] - BOX[2][0]) < 0.01)) | (outside & (np.abs(P[:, 2] - Z0) < 0.01))
    print("vertices %d, coloured %d, on the surface %d, coloured there %d" % (len(P), got["colored"].sum(), on.sum(), (got["colored"] & on).sum()))
    assert on.sum() > 4000 and got["colored"][on].all() and got["counts"][0] == got["colored"].sum() >= 0.95 * len(P)
    err = got["bgr"][on].astype(np.float64) - texture(P[on])
    assert np.sqrt(np.mean(err ** 2)) < NOISE / np.sqrt(3.0)  # better than one noisy image's 11.5 levels
    assert np.array_equal(got["bgr8"][on], np.clip(np.rint(got["bgr"][on]), 0, 255).astype(np.uint8))


# ---- 3. the sampler's edges ----------------------------------------------------------------------------------------------------
def small_volume(n=(5, 4, 3), seed=4):
    grid = TR.make_grid(*n, (-0.02, 0.01, 1.0), 0.01, 0.04)
    rng = np.random.default_rng(seed)
    col = np.zeros((n[2], n[1], n[0], 4), np.float32)
    col[..., :3] = rng.uniform(0, 255, col.shape[:3] + (3,))
    col[..., 3] = 1.0
    return grid, col


def at(grid, q):
    """The binary32 world position of grid coordinates q (exact for the few values used here is not needed: the test reads
    the coordinates back through the definition)."""
    return (np.array(grid["origin"]) + np.asarray(q, np.float64) * grid["voxel"]).astype(np.float32)


def test_definition_the_sampler_at_the_grids_edges():
    grid, col = small_volume()
    nx, ny, nz = grid["nx"], grid["ny"], grid["nz"]
    s = lambda q, c=col, g=grid, mw=0.0: [a[0] for a in CR.sample(g, c, mw, *[np.array([v], np.float64) for v in q])]
    # exactly on the last node plane of every axis: the corners beyond it are never read, the node itself answers
    ok, value, den, parts = s((nx - 1.0, ny - 1.0, nz - 1.0))
    assert ok and parts == 1 and den == 1.0 and np.array_equal(bits(value), bits(col[nz - 1, ny - 1, nx - 1, :3]))
    ok, value, den, parts = s((nx - 1.0, 1.5, 0.25))
    assert ok and parts == 4 and den == 1.0
    # a binary32 ulp outside the grid, as a mesh vertex rounded to float may lie: still coloured, from the nodes of that face
    P = at(grid, (nx - 1.0, 1.0, 1.0))
    P[0] = np.nextafter(P[0], np.float32(np.inf))
    q = [v[0] for v in CR.point_coordinates(grid, P)]
    assert q[0] > nx - 1 and q[0] - (nx - 1) < 1e-3
    got = CR.color_points(grid, col, P[None, :])
    assert got["colored"][0] and got["parts"][0] >= 1 and np.abs(got["bgr"][0] - col[1, 1, nx - 1, :3]).max() < 0.5
    ok, _, _, parts = s((-1e-9, 1.0, 1.0))  # a hair below the first plane: lo = -1, only the corners of plane 0 lie inside
    assert ok and 1 <= parts <= 4
    # a grid one node thick
    thin, tcol = small_volume((5, 4, 1))
    ok, value, den, parts = s((1.5, 2.0, 0.0), tcol, thin)
    assert ok and parts == 4 and den == 1.0  # the row y = 3 takes part with tw = 0; the slice z = 1 does not exist
    want =(np.float32(0.5) * tcol[0, 2, 1, :3]) + (np.float32(0.5) * tcol[0, 2, 2, :3])
    assert np.array_equal(bits(value), bits(want.astype(np.float32)))
    one, ocol = small_volume((1, 1, 1))
    ok, value, _, parts = s((0.0, 0.0, 0.0), ocol, one)
    assert ok and parts == 1 and np.array_equal(bits(value), bits(ocol[0, 0, 0, :3]))
    # far outside, and what is no position at all
    for q in ((nx + 0.5, 1.0, 1.0), (-1.5, 1.0, 1.0), (1.0, 1.0, 1e9), (2.0 ** 30, 1.0, 1.0), (np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (1.0, 1.0, -np.inf)):
        ok, value, den, parts = s(q)
        assert not ok and parts == 0 and (bits(value) == 0).all(), q
    assert s((2.0 ** 30 - 1, 1.0, 1.0))[3] == 0
    got = CR.color_points(grid, col, np.array([[1e30, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], np.float32), byte_scale=255.0)
    assert got["counts"][0] == 0 and (got["bgr8"] == 0).all() and (bits(got["bgr"]) == 0).all()


def test_definition_one_corner_min_weight_and_records_that_take_no_part():
    grid, col = small_volume()
    s = lambda q, c, mw=0.0: [a[0] for a in CR.sample(grid, c, mw, *[np.array([v], np.float64) for v in q])]
    lone = np.zeros_like(col)
    lone[1, 2, 3] = col[1, 2, 3]
    # one participating corner returns that corner's colour: exactly where tw is a power of two ((tw * C) / tw) ...
    for q in ((2.5, 1.5, 0.5), (3.0, 2.0, 1.0), (2.75, 2.0, 1.0), (3.5, 2.5, 1.25)):
        ok, value, den, parts = s(q, lone)
        assert ok and parts == 1 and np.array_equal(bits(value), bits(col[1, 2, 3, :3])), q
    # ... and within a rounding of the product and one of the quotient for any tw
    rng = np.random.default_rng(6)
    for _ in range(50):
        q = np.array([2, 1, 0]) + rng.uniform(0.05, 0.95, 3)
        ok, value, den, parts = s(q, lone)
        assert ok and parts == 1 and (np.abs(value - col[1, 2, 3, :3]) <= np.spacing(col[1, 2, 3, :3])).all()
    ok, _, _, parts = s((3.0, 2.0, 1.0), np.zeros_like(col))
    assert not ok and parts == 0  # never coloured
    # on the node whose only coloured neighbour has tw = 0: den = 0, not coloured
    ok, _, den, parts = s((2.0, 2.0, 1.0), lone)
    assert not ok and parts == 1 and den == 0.0
    # min_weight: a corner takes part iff weight > 0 and weight >= min_weight
    heavy = col.copy()
    heavy[..., 3] = 1.0
    heavy[1, 2, 3, 3] = 2.0
    ok, value, _, parts = s((2.5, 1.5, 0.5), heavy, 2.0)
    assert ok and parts == 1 and np.array_equal(bits(value), bits(col[1, 2, 3, :3]))
    assert s((2.5, 1.5, 0.5), heavy, 1.0)[3] == 8 and s((2.5, 1.5, 0.5), heavy, 2.5)[3] == 0
    # a weight that is negative, -0.0 or NaN and a channel that is not finite take no part
    for word, value in ((3, -1.0), (3, -0.0), (3, np.nan), (0, np.nan), (1, np.inf), (2, -np.inf)):
        broken = col.copy()
        broken[1, 2, 3, word] = value
        assert s((2.5, 1.5, 0.5), broken)[3] == 7, (word, value)
    # the bytes: rintf half to even, saturated either side
    ok, value = np.array([True] * 5), np.array([[0.5, 1.5, 2.5], [-3.0, 254.5, 255.5], [1e9, -1e9, 254.49], [np.inf, -np.inf, 3.0], [0.0, -0.0, 1.0]], np.float32)
    assert np.array_equal(CR.outputs(ok, value, 1.0)[1], np.array([[0, 2, 2], [0, 254, 255], [255, 0, 254], [255, 0, 3], [0, 0, 1]], np.uint8))
    assert np.array_equal(CR.outputs(ok, value, 255.0)[1][4], np.array([0, 0, 255], np.uint8))


# ---- the cases the kernels are held to ------------------------------------------------------------------------------------------
def case_points(grid, n, seed):
    """n world-frame points: most inside the grid or within a voxel of it, every fourth exactly on a node, the last nodes' planes
    and positions that are none (NaN, +-inf, 1e30) among them."""
    rng = np.random.default_rng(seed)
    dims = np.array([grid["nx"], grid["ny"], grid["nz"]])
    q = rng.uniform(-1.0, dims, (n, 3))
    q[::4] = np.rint(q[::4])
    if n > 8:
        q[1] = dims - 1
        q[2] = (0, 0, 0)
    P = (np.array(grid["origin"]) + q * grid["voxel"]).astype(np.float32)
    if n > 8:
        P[3, 0], P[5, 1], P[6, 2], P[7] = np.nan, np.inf, -np.inf, 1e30
    return P


@functools.lru_cache(maxsize=None)
def color_case(volume, shape, pose="identity", map_pose=None, float_image=False, weighted=False, band=1.0, min_weight=0.0,
               byte_scale=1.0, n=65, d_n=None, history=False, max_weight=64.0, seed=0):
    """One integrate into the cleared volumes (or into volumes with a history), then both gathers on what it left -> (the
    arguments of check_color as a dict, the definition's results)."""
    rows, cols = MAPS[shape]
    grid = case_grid(volume, max_weight)
    camera = case_camera(shape, pose == "identity")
    p, dist = case_pose(grid, pose)
    rng = np.random.default_rng(1000 + seed + rows + cols)
    disp = case_map(shape, camera, dist, seed=rows + cols + seed)
    weight = FT.random_weight(np.random.default_rng(100 + seed), rows, cols) if weighted else None
    if float_image:
        image = rng.uniform(0.0, 1.0, (rows, cols, 3)).astype(np.float32)
        if image.size > 60:
            image.ravel()[7:60:11] = (np.nan, np.inf, -np.inf, -0.0, 1e-40)
    else:
        image = rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8)
    shape3 = (grid["nz"], grid["ny"], grid["nx"])
    voxels, colors = TR.clear(grid), CR.clear(grid)
    run = lambda c: CR.integrate(grid, voxels, c, disp, image, camera, *p, weight=weight, band=band)
    if history:  # random values and weights, and NaN payloads in records that the integrate leaves untouched
        voxels = rng.uniform(-1, 1, shape3 + (2,)).astype(np.float32)
        voxels[..., 1] = rng.choice([0.0, 1.0, 2.0, 3.5], shape3)
        colors = rng.uniform(0, 255, shape3 + (4,)).astype(np.float32)
        colors[..., 3] = rng.choice([0.0, 1.0, 2.0, 3.5], shape3)
        untouched = np.argwhere(~run(colors)["colored"])
        for k, words in enumerate(((0x7FC00001, 0xFFC00000, 0x7F800001, 0x3F800000), (0, 0x7FFFFFFF, 0, 0x40000000))):
            if len(untouched) > 7 * k + 3:
                colors.view(np.uint32)[tuple(untouched[7 * k + 3])] = words
    want = run(colors)
    mp, mdist = case_pose(grid, map_pose or pose)
    map_disp = disp if map_pose is None else case_map(shape, camera, mdist, seed=rows + cols + seed + 1)
    want_map = CR.color_map(grid, want["colors"], map_disp, camera, *mp, min_weight=min_weight, byte_scale=byte_scale)
    xyz = case_points(grid, n, seed + 5)
    start_bgr = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    start_bgr8 = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    limit = None if d_n is None else d_n
    want_pts = CR.color_points(grid, want["colors"], xyz, min_weight, byte_scale, limit, start_bgr, start_bgr8)
    args = dict(grid=grid, camera=camera, pose=p, map_pose=mp, rows=rows, cols=cols, disp=disp, weight=weight, image=image, band=band,
                min_weight=min_weight, byte_scale=byte_scale, voxels=voxels, colors=colors, map_disp=map_disp, xyz=xyz, d_n=d_n,
                start_bgr=start_bgr, start_bgr8=start_bgr8)
    return args, dict(integrate=want, map=want_map, points=want_pts)


def test_conditions_the_cases_colour_and_gather():
    """The cases below do reach the code they are for: both spans of a 70-voxel row are coloured, the band excludes voxels, the
    maps and the point lists are coloured in part, and the history leaves records with NaN payloads untouched."""
    args, want = color_case("70x9x5", "9x300")
    col = want["integrate"]["colored"]
    assert col[..., :64].any() and col[..., 64:].any()
    cols_hit = np.flatnonzero(want["map"]["colored"].any(0))
    assert cols_hit.min() < 128 and cols_hit.max() >= 192  # across wavefronts of the map gather
    _, narrow = color_case("37x21x13", "37x53", band=0.25)
    _, wide = color_case("37x21x13", "37x53")
    assert 100 < narrow["integrate"]["counts"][2] < wide["integrate"]["counts"][2] <= wide["integrate"]["counts"][1]
    assert 0 < wide["map"]["counts"][0] < 37 * 53
    _, pts = color_case("37x21x13", "37x53", n=1000)
    assert 100 < pts["points"]["counts"][0] < 1000 and (pts["points"]["parts"] == 8).any() and (pts["points"]["parts"] == 1).any()
    args, hist = color_case("37x21x13", "37x53", history=True, weighted=True)
    assert np.isnan(hist["integrate"]["colors"]).sum() >= 4 and hist["integrate"]["counts"][2] > 100
    for volume in ("1x1x1", "1x7x3"):
        _, thin = color_case(volume, "37x53")
        assert thin["integrate"]["counts"][2] >= 1 and thin["map"]["counts"][0] >= 1
    for pose in ("behind", "beside"):
        _, none = color_case("37x21x13", "37x53", pose=pose)
        assert tuple(none["integrate"]["counts"]) == (0, 0, 0) and none["map"]["counts"][0] == 0


# ---- 4. the kernels' own per-thread code, run on the host ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_color_exe(tmp_path_factory):
    """tests/cpp/tsdf_color_host_main.cpp: csrc/pm_tsdf_color_body.hpp compiled for the host alone, with the sanitizers."""
    return build_host_kernel(tmp_path_factory.mktemp("tsdfcolorhost") / "tsdf_color_host_main", "tsdf_color_host_main.cpp")


def _dump(path, args, want):
    g = args["grid"]
    rows, cols = args["rows"], args["cols"]
    w = args["weight"]
    dump_case(path, [g["nx"], g["ny"], g["nz"], *g["origin"], g["voxel"], g["trunc"], g["max_weight"], *args["camera"], rows, cols, 0.0,
                     0.0, args["band"], w is not None, args["image"].dtype != np.uint8, args["min_weight"], args["byte_scale"],
                     len(args["xyz"]), 2.0 ** 31 if args["d_n"] is None else args["d_n"],
                     *np.asarray(args["pose"][0]).ravel(), *np.asarray(args["pose"][1]).ravel(),
                     *np.asarray(args["map_pose"][0]).ravel(), *np.asarray(args["map_pose"][1]).ravel()],
              start_voxels=args["voxels"], start_colors=args["colors"], disp=args["disp"],
              weights=w if w is not None else np.full((rows, cols), 7.0, np.float32), image=args["image"], map_disp=args["map_disp"],
              xyz=args["xyz"], start_bgr=args["start_bgr"], start_bgr8=args["start_bgr8"],
              want_voxels=want["integrate"]["voxels"], want_colors=want["integrate"]["colors"], want_counts=want["integrate"]["counts"],
              want_map_bgr=want["map"]["bgr"], want_map_bgr8=want["map"]["bgr8"], want_map_count=want["map"]["counts"],
              want_pts_bgr=want["points"]["bgr"], want_pts_bgr8=want["points"]["bgr8"], want_pts_count=want["points"]["counts"])


POSES = ("identity", "yaw", "roll", "inside", "behind", "beside")
COLOR_MAPS = ("1x1", "37x53", "9x300")
POINT_COUNTS = (0, 1, 63, 64, 65, 1000)


def test_kernel_code_on_the_host_equals_the_definition(host_color_exe, tmp_path):
    """Every thread of the three launches over whole volumes, maps and point lists on the CPU, forwards and backwards, each gather
    with each output alone and with the count alone: both volumes, the counts and every output equal the .npy dumps of the
    definition byte for byte, and AddressSanitizer / UBSan see every access into buffers of exactly the size a stage may touch.
    Four volumes x three maps, the poses and the point counts in turn, byte and float images, weights given and null, band 0.25
    and 1, min_weight 0 and 2, byte_scale 1 and 255, d_n absent, smaller and larger than n, and volumes with a history."""
    totals, k, d = np.zeros(5, np.int64), 0, None
    for volume in VOLUMES:
        for shape in COLOR_MAPS:
            n = POINT_COUNTS[k % len(POINT_COUNTS)]
            args, want = color_case(volume, shape, pose=POSES[k % len(POSES)], map_pose=(None, "yaw", "roll")[k % 3],
                                    float_image=k % 2 == 1, weighted=k % 3 == 1, band=(1.0, 0.25)[k % 2], min_weight=(0.0, 2.0)[k % 4 == 3],
                                    byte_scale=(1.0, 255.0)[k % 2], n=n, d_n=(None, n // 2, n + 7)[k % 3], history=k % 4 >= 2,
                                    max_weight=(64.0, 1.5)[k % 5 == 4])
            d = str(tmp_path / ("case%d" % k))
            _dump(d, args, want)
            r = subprocess.run([host_color_exe, d], capture_output=True, text=True)
            assert r.returncode == 0, (volume, shape, k, r.stderr[-3000:])
            totals += (*want["integrate"]["counts"], want["map"]["counts"][0], want["points"]["counts"][0])
            k += 1
    # a *d_n < 0 counts as 0: no point is worked on, every output keeps its bytes
    args, want = color_case("37x21x13", "37x53", n=65, d_n=-3)
    assert want["points"]["counts"][0] == 0 and np.array_equal(bits(want["points"]["bgr"]), bits(args["start_bgr"]))
    d = str(tmp_path / "negative")
    _dump(d, args, want)
    r = subprocess.run([host_color_exe, d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    args, want = color_case("37x21x13", "37x53", pose="yaw", map_pose="roll", weighted=True, n=1000, d_n=900, history=True)
    d = str(tmp_path / "history")
    _dump(d, args, want)
    r = subprocess.run([host_color_exe, d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    print("in view, updated, coloured, pixels, points:", totals, want["map"]["counts"], want["points"]["counts"])
    assert totals[2] > 3000 and totals[3] > 300 and totals[4] > 100 and want["map"]["counts"][0] > 100 and want["points"]["counts"][0] > 100
    # the program does compare: one flipped bit in an expectation is a mismatch, not a pass
    assert_program_compares(host_color_exe, d,
                            [("want_" + name, dtype, word + " differs") for name, dtype, word in
                             (("voxels", np.uint32, "the distance volume"), ("colors", np.uint32, "the colour volume"),
                              ("counts", np.int32, "the integrate's counts"), ("map_bgr", np.uint32, "the map's floats"),
                              ("map_bgr8", np.uint8, "the map's bytes"), ("map_count", np.int32, "the map's count"),
                              ("pts_bgr", np.uint32, "the points' floats"), ("pts_bgr8", np.uint8, "the points' bytes"),
                              ("pts_count", np.int32, "the points' count"))])


def test_headers_declare_and_the_library_exports_the_colour_functions(pm):
    text = open(os.path.join(ROOT, "include", "pm", "imaging.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = pm.load()
    assert re.search(r"\bsize_t\s+pm_tsdf_color_bytes\s*\(\s*const\s+pm_tsdf_volume\s*\*", text)
    for name in ("pm_tsdf_color_clear", "pm_tsdf_integrate_color", "pm_tsdf_color_map", "pm_tsdf_color_points"):
        assert re.search(r"\bint\s+%s\s*\(\s*pm_handle\s*\*" % name, text), name
        assert name in pm.EXPORTS and hasattr(lib, name), name
    for name in ("pm_tsdf_color_bytes", "pm_debug_tsdf_color_constants"):
        assert name in pm.EXPORTS and hasattr(lib, name), name
    for name in ("pm_tsdf_color_options", "pm_tsdf_color_sample_options"):
        assert "typedef struct " + name in text, name
    assert text.index("pm_motion_compose") < text.index("pm_tsdf_color_bytes") < text.index("pm_tsdf_color_points") < text.index("pm_device_malloc")
    assert "#define PM_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "pm", "patchmatch.h")).read() and pm.PM_ABI_VERSION == 6
    assert (C.sizeof(pm.PmTsdfColorOptions), C.sizeof(pm.PmTsdfColorSampleOptions)) == (12, 8)
    assert pm.tsdf_color_constants() == (16,) + pm.tsdf_constants()
    assert pm.tsdf_color_bytes(GRID) == 16 * 52 * 34 * 40 == 2 * pm.tsdf_bytes(GRID) and lib.pm_tsdf_color_bytes(None) == 0
    for bad in (dict(nx=0), dict(voxel=0.0), dict(trunc=float("nan")), dict(max_weight=0.0), dict(nx=2048, ny=2048, nz=512)):
        assert pm.tsdf_color_bytes(dict(GRID, **bad)) == 0 == pm.tsdf_bytes(dict(GRID, **bad)), bad
    csrc = os.path.join(ROOT, "ocean-perception_amd", "csrc")
    assert '#include "pm_tsdf_color.hpp"' in open(os.path.join(csrc, "pm_stages.hip")).read()
    assert "pm_tsdf_color.hpp" in open(os.path.join(csrc, "pm_handle.hpp")).read()
    body = open(os.path.join(csrc, "pm_tsdf_color_body.hpp")).read()
    assert "__global__" not in body and "tsdf_integrate_lane(a.base" in body  # host-callable; the distance statement is shared


# ---- 5. device parity ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        yield e


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    g = got.view(np.uint32) if got.dtype == np.float32 else got
    w = want.view(np.uint32) if want.dtype == np.float32 else want
    bad = np.argwhere(g.reshape(w.shape) != w)
    assert len(bad) == 0, "%s: %d of %d values differ; (index, got, want): %s" % (
        what, len(bad), w.size, [(tuple(map(int, b)), got.reshape(want.shape)[tuple(b)], want[tuple(b)]) for b in bad[:6]])


def check_color(torch, e, args, want, outputs=("bgr", "bgr8", "d_counts", "counts"), offset_floats=0, clear=False):
    """One case on the device against the definition: the integrate (both volumes, d_counts and host counts), then the map gather
    and the point gather with the `outputs` asked for.  clear: the volumes start as patterned buffers that pm_tsdf_clear and
    pm_tsdf_color_clear run over (the case's start must be the cleared one).  offset_floats: the maps and the float outputs start
    that many floats past a 16-byte boundary.  Guard bands around everything the stages write."""
    import pm_ctypes as pm
    g, rows, cols = args["grid"], args["rows"], args["cols"]
    vox, px, n = g["nx"] * g["ny"] * g["nz"], rows * cols, len(args["xyz"])
    off = 4 * offset_floats
    assert pm.tsdf_color_bytes(g) == 16 * vox
    volume, colors = FT.Guarded(torch, 8 * vox), FT.Guarded(torch, 16 * vox)
    assert colors.ptr % 16 == 0
    if clear:
        volume.t[volume.lo:volume.lo + volume.n] = 0x5A
        colors.t[colors.lo:colors.lo + colors.n] = 0x5A
        torch.cuda.synchronize()
        e.tsdf_clear(g, volume.ptr)
        e.tsdf_color_clear(g, colors.ptr)
    else:
        volume.t[volume.lo:volume.lo + volume.n] = torch.from_numpy(args["voxels"].view(np.uint8).ravel())
        colors.t[colors.lo:colors.lo + colors.n] = torch.from_numpy(args["colors"].view(np.uint8).ravel())

    def up(a, dtype=np.float32, shift=offset_floats):
        a = np.ascontiguousarray(a, dtype).ravel()
        t = torch.zeros(a.size + shift + 1, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
        t[shift:shift + a.size] = torch.from_numpy(a)
        return t, t.data_ptr() + shift * a.itemsize

    d, d_ptr = up(args["disp"])
    w = up(args["weight"]) if args["weight"] is not None else None
    byte_image = args["image"].dtype == np.uint8
    image = up(args["image"], args["image"].dtype, offset_floats if not byte_image else (1 if offset_floats else 0))
    cnt = FT.Guarded(torch, 12) if "d_counts" in outputs else None
    torch.cuda.synchronize()  # the uploads run on torch's stream, the stages on the handle's
    got = e.tsdf_integrate_color(args["camera"], g, args["pose"], d_ptr, rows, cols, volume.ptr, colors.ptr,
                                 d_bgr8=image[1] if byte_image else None, d_bgr=None if byte_image else image[1], band=args["band"],
                                 d_weight=w[1] if w else None, d_counts=cnt.ptr if cnt else None, want_counts="counts" in outputs)
    e.synchronize()
    wi = want["integrate"]
    if "counts" in outputs:
        assert tuple(got) == tuple(int(v) for v in wi["counts"]), (got, wi["counts"])
    else:
        assert got is None
    if cnt:
        assert np.array_equal(cnt.read(np.int32), wi["counts"])
    _same("the distance volume", volume.read(np.float32).reshape(wi["voxels"].shape), wi["voxels"])
    _same("the colour volume", colors.read(np.float32).reshape(wi["colors"].shape), wi["colors"])
    # the map gather
    md, md_ptr = up(args["map_disp"])
    out = FT.Guarded(torch, 12 * px, off) if "bgr" in outputs else None
    out8 = FT.Guarded(torch, 3 * px, 1 if offset_floats else 0) if "bgr8" in outputs else None
    cnt = FT.Guarded(torch, 4) if "d_counts" in outputs else None
    torch.cuda.synchronize()
    got = e.tsdf_color_map(args["camera"], g, args["map_pose"], colors.ptr, md_ptr, rows, cols, args["min_weight"], args["byte_scale"],
                           out.ptr if out else None, out8.ptr if out8 else None, cnt.ptr if cnt else None, "counts" in outputs)
    e.synchronize()
    wm = want["map"]
    assert got == (int(wm["counts"][0]) if "counts" in outputs else None), (got, wm["counts"])
    if cnt:
        assert np.array_equal(cnt.read(np.int32), wm["counts"])
    if out:
        _same("the map's floats", out.read(np.float32).reshape(rows, cols, 3), wm["bgr"])
    if out8:
        _same("the map's bytes", out8.read(np.uint8).reshape(rows, cols, 3), wm["bgr8"])
    # the point gather: its outputs hold values, which the points behind min(n, *d_n) keep
    x, x_ptr = up(args["xyz"])
    out = FT.Guarded(torch, 12 * n, off) if "bgr" in outputs else None
    out8 = FT.Guarded(torch, 3 * n, 1 if offset_floats else 0) if "bgr8" in outputs else None
    if out and n:
        out.t[out.lo:out.lo + out.n] = torch.from_numpy(args["start_bgr"].view(np.uint8).ravel())
    if out8 and n:
        out8.t[out8.lo:out8.lo + out8.n] = torch.from_numpy(args["start_bgr8"].ravel())
    cnt = FT.Guarded(torch, 4) if "d_counts" in outputs else None
    d_n = torch.tensor([args["d_n"]], dtype=torch.int32, device="cuda") if args["d_n"] is not None else None
    torch.cuda.synchronize()
    got = e.tsdf_color_points(g, colors.ptr, x_ptr, n, args["min_weight"], args["byte_scale"], d_n.data_ptr() if d_n is not None else None,
                              out.ptr if out else None, out8.ptr if out8 else None, cnt.ptr if cnt else None, "counts" in outputs)
    e.synchronize()
    wp = want["points"]
    assert got == (int(wp["counts"][0]) if "counts" in outputs else None), (got, wp["counts"])
    if cnt:
        assert np.array_equal(cnt.read(np.int32), wp["counts"])
    if out:
        _same("the points' floats", out.read(np.float32).reshape(n, 3), wp["bgr"])
    if out8:
        _same("the points' bytes", out8.read(np.uint8).reshape(n, 3), wp["bgr8"])
    _same("the colour volume behind the gathers", colors.read(np.float32).reshape(wi["colors"].shape), wi["colors"])
    for t, a in ((d, args["disp"]), (md, args["map_disp"])):
        assert np.array_equal(bits(t.cpu().numpy()[offset_floats:offset_floats + px]), bits(a).ravel()), "a stage wrote to its input map"
    return want


@gpu
@pytest.mark.parametrize("shape", COLOR_MAPS)
@pytest.mark.parametrize("volume", list(VOLUMES))
def test_colour_equals_the_definition(pm, engine, volume, shape):
    """Four volumes (one voxel; one node thick along x; a row that crosses the 64-voxel span and leaves a tail of 6; several
    spans, rows and slices) x three maps (one pixel; rows that are no multiple of the block's 4; a row of five wavefronts with a
    ragged tail): both clears over patterned buffers, then a byte image at band 1 and, into volumes with a history -- random
    colours and weights, NaN payloads in records that stay untouched --, a float image with weights at band 0.25, gathered from
    another pose with min_weight 2 and byte_scale 255."""
    import torch
    check_color(torch, engine, *color_case(volume, shape), clear=True)
    check_color(torch, engine, *color_case(volume, shape, pose="yaw", map_pose="roll", float_image=True, weighted=True, band=0.25,
                                           min_weight=2.0, byte_scale=255.0, history=True, n=64, d_n=40))


@gpu
@pytest.mark.parametrize("pose", POSES)
def test_every_pose(pm, engine, pose):
    """The camera in front of the volume, yawed, rolled, inside it, behind it and beside it: integrated from there, the map
    gathered from there, bytes and floats."""
    import torch
    want = check_color(torch, engine, *color_case("37x21x13", "37x53", pose=pose, weighted=True))
    assert (want["integrate"]["counts"][2] > 0) == (pose not in ("behind", "beside"))
    check_color(torch, engine, *color_case("70x9x5", "9x300", pose=pose, float_image=True, band=0.25, byte_scale=255.0))


@gpu
@pytest.mark.parametrize("d_n", ["absent", "smaller", "larger", "negative"])
@pytest.mark.parametrize("n", POINT_COUNTS)
def test_point_counts(pm, engine, n, d_n):
    """n of 0, 1, one short of a wavefront, a wavefront, one more, and four blocks with a tail; d_n absent, smaller than n and
    larger than n: the points behind min(n, *d_n) keep their output bytes.  A *d_n < 0 counts as 0."""
    import torch
    limit = {"absent": None, "smaller": n // 2, "larger": n + 7, "negative": -3}[d_n]
    want = check_color(torch, engine, *color_case("37x21x13", "37x53", n=n, d_n=limit, history=True, min_weight=(0.0, 2.0)[n % 2]))
    m = max(0, min(n, n if limit is None else limit))
    assert want["points"]["counts"][0] <= m and (want["points"]["counts"][0] > 0 or m < 31)


@gpu
def test_each_output_alone_unaligned_and_the_options(pm, engine):
    """Each output of the gathers absent in turn and each alone; maps, images and float outputs 4, 8 and 12 bytes past a 16-byte
    boundary (the byte streams one byte past it); band, min_weight, byte_scale, weights and a max_weight that saturates."""
    import torch
    four = ("bgr", "bgr8", "d_counts", "counts")
    case = color_case("37x21x13", "37x53", pose="roll", weighted=True, n=1000, d_n=700)
    for outputs in [tuple(k for k in four if k != drop) for drop in four] + [(k,) for k in four]:
        check_color(torch, engine, *case, outputs=outputs)
    for off in (1, 2, 3):
        check_color(torch, engine, *color_case("70x9x5", "9x300", float_image=off != 2, weighted=True, n=65), offset_floats=off)
    for band in (0.25, 1.0):
        for min_weight in (0.0, 2.0):
            for byte_scale in (1.0, 255.0):
                check_color(torch, engine, *color_case("37x21x13", "37x53", pose="yaw", float_image=byte_scale == 255.0, band=band,
                                                       min_weight=min_weight, byte_scale=byte_scale, history=True, weighted=band == 1.0))
    want = check_color(torch, engine, *color_case("37x21x13", "37x53", max_weight=1.5, weighted=True, history=True))
    assert want["integrate"]["colors"][..., 3][want["integrate"]["colored"]].max() == 1.5


@gpu
def test_the_distance_volume_is_pm_tsdf_integrates_own(pm, engine):
    """pm_tsdf_integrate and pm_tsdf_integrate_color from the same start and the same arguments: the distance volumes and the
    first two counts are the same bytes."""
    import torch
    args, want = color_case("37x21x13", "37x53", pose="yaw", weighted=True, history=True, band=0.25)
    g, rows, cols = args["grid"], args["rows"], args["cols"]
    vox = 37 * 21 * 13
    a, b, colors = FT.Guarded(torch, 8 * vox), FT.Guarded(torch, 8 * vox), FT.Guarded(torch, 16 * vox)
    for buf in (a, b):
        buf.t[buf.lo:buf.lo + buf.n] = torch.from_numpy(args["voxels"].view(np.uint8).ravel())
    colors.t[colors.lo:colors.lo + colors.n] = torch.from_numpy(args["colors"].view(np.uint8).ravel())
    d, w = (torch.from_numpy(args[k]).cuda() for k in ("disp", "weight"))
    image = torch.from_numpy(args["image"]).cuda()
    ca, cb = FT.Guarded(torch, 8), FT.Guarded(torch, 12)
    torch.cuda.synchronize()
    na = engine.tsdf_integrate(args["camera"], g, args["pose"], d.data_ptr(), rows, cols, a.ptr, d_weight=w.data_ptr(), d_counts=ca.ptr,
                               want_counts=True)
    nb = engine.tsdf_integrate_color(args["camera"], g, args["pose"], d.data_ptr(), rows, cols, b.ptr, colors.ptr, d_bgr8=image.data_ptr(),
                                     band=0.25, d_weight=w.data_ptr(), d_counts=cb.ptr, want_counts=True)
    engine.synchronize()
    assert tuple(na) == tuple(nb[:2]) == tuple(want["integrate"]["counts"][:2]) and nb[1] > nb[2] > 100
    assert np.array_equal(ca.read(np.int32), cb.read(np.int32)[:2])
    va, vb = a.read(np.uint32), b.read(np.uint32)
    assert np.array_equal(va, vb) and np.array_equal(va, bits(want["integrate"]["voxels"]).ravel())
    assert not np.array_equal(va, bits(args["voxels"]).ravel())


@gpu
@pytest.mark.parametrize("mode", ["scalar", "planes"])
def test_colour_directly_behind_a_match_and_a_mesh_on_the_handles_stream(pm, synth, mode):
    """A Match() of a synthetic pair into a device buffer, then both clears, pm_tsdf_integrate_color with the left image's bytes
    as its colour, pm_tsdf_mesh and pm_tsdf_color_points with the mesh's DEVICE vertex count as d_n, on the handle's stream with
    nothing copied and nothing synchronised in between: everything equals the definition on the downloaded disparity map."""
    import torch
    rows, cols = 96, 128
    cam = (100.0, 100.0, 64.0, 48.0, 0.02)
    kw = dict(mode=pm.PM_MODE_PLANES) if mode == "planes" else {}
    p = synth.make_pair(5, rows=rows, cols=cols, n_points=40, dilate_factor=2)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    L, R, SL, SR = (up(p[k]) for k in ("left", "right", "seed_l", "seed_r"))
    image_host = np.repeat(p["left"][..., None], 3, -1).astype(np.uint8)
    image_host[..., 1] = 255 - image_host[..., 1]
    image = up(image_host)
    D = torch.zeros((2, rows, cols), dtype=torch.float32, device="cuda")
    grid = TR.make_grid(40, 32, 40, (-0.5, -0.4, 0.05), 0.025, 0.1, 8.0)
    vox, cap = 40 * 32 * 40, 60000
    vol, col = FT.Guarded(torch, 8 * vox), FT.Guarded(torch, 16 * vox)
    for buf in (vol, col):
        buf.t[buf.lo:buf.lo + buf.n] = 0x5A
    xyz, out, out8 = FT.Guarded(torch, 12 * cap), FT.Guarded(torch, 12 * cap), FT.Guarded(torch, 3 * cap)
    counts, colored = FT.Guarded(torch, 8), FT.Guarded(torch, 4)
    torch.cuda.synchronize()
    with pm.Engine(pm.default_params(0, patch=5, patchmatch_iters=2, max_disp=32, **kw), max_rows=rows, max_cols=cols) as e:
        e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), D[0].data_ptr(), D[1].data_ptr())
        e.tsdf_clear(grid, vol.ptr)
        e.tsdf_color_clear(grid, col.ptr)
        e.tsdf_integrate_color(cam, grid, IDENT, D[0].data_ptr(), rows, cols, vol.ptr, col.ptr, d_bgr8=image.data_ptr(), band=0.5)
        e.tsdf_mesh(grid, vol.ptr, cap, 0, d_xyz_out=xyz.ptr, d_counts=counts.ptr, want_counts=False)
        e.tsdf_color_points(grid, col.ptr, xyz.ptr, cap, byte_scale=1.0, d_n=counts.ptr, d_bgr_out=out.ptr, d_bgr8_out=out8.ptr,
                            d_counts=colored.ptr)
        e.synchronize()
    disp = D[0].cpu().numpy()
    want = CR.integrate(grid, TR.clear(grid), CR.clear(grid), disp, image_host, cam, *IDENT, band=0.5)
    mesh = MR.mesh(grid, want["voxels"])
    n = int(mesh["counts"][0])
    pts = CR.color_points(grid, want["colors"], mesh["xyz"], byte_scale=1.0)
    print(mode, "updated, coloured", want["counts"][1:], "vertices", n, "coloured", pts["counts"])
    assert 100 < n <= cap and want["counts"][2] > 100 and pts["counts"][0] > 0
    assert np.array_equal(vol.read(np.uint32), bits(want["voxels"]).ravel())
    assert np.array_equal(col.read(np.uint32), bits(want["colors"]).ravel())
    assert counts.read(np.int32)[0] == n and colored.read(np.int32)[0] == pts["counts"][0]
    assert np.array_equal(xyz.read(np.uint32, 12 * n), bits(mesh["xyz"]).ravel())
    assert np.array_equal(out.read(np.uint32, 12 * n), bits(pts["bgr"]).ravel())  # nothing behind the device count is written
    assert np.array_equal(out8.read(np.uint8, 3 * n), pts["bgr8"].ravel())


# ---- 6. refusals: the order of the checks and the whole texts ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch
    rows, cols = 16, 24
    maps = dict(disp=torch.full((rows, cols), 4.25, dtype=torch.float32, device="cuda"),
                vol=torch.zeros(2 * 64, dtype=torch.float32, device="cuda"), col=torch.zeros(4 * 64, dtype=torch.float32, device="cuda"),
                bgr8=torch.zeros((rows, cols, 3), dtype=torch.uint8, device="cuda"),
                bgr=torch.zeros((rows, cols, 3), dtype=torch.float32, device="cuda"),
                out=torch.zeros((rows, cols, 3), dtype=torch.float32, device="cuda"), xyz=torch.zeros((8, 3), dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    ptr = {k: v.data_ptr() for k, v in maps.items()}
    ptr["keep"] = maps
    return ptr


SAMPLE_FIELDS = ("min_weight", "byte_scale")


def sample_steps(pm):
    """min_weight = -1 and byte_scale = inf at the start."""
    E = pm.PM_ERR_INVALID_ARG
    return [(E, "min_weight must not be NaN or negative", fix("options", "min_weight", NAN)),
            (E, "min_weight must not be NaN or negative", fix("options", "min_weight", 0.0)),
            (E, "byte_scale must be finite and > 0", fix("options", "byte_scale", 0.0)),
            (E, "byte_scale must be finite and > 0", fix("options", "byte_scale", NAN)),
            (E, "byte_scale must be finite and > 0", fix("options", "byte_scale", 255.0))]


@gpu
def test_refusals_of_color_clear(pm, engine, dev):
    E = pm.PM_ERR_INVALID_ARG
    a = dict(volume=None, d_colors=None)
    call = lambda lib, h, a: lib.pm_tsdf_color_clear(h, c_volume(pm, a["volume"]), a["d_colors"])
    steps = ([(E, "null volume", fix("volume", copy.deepcopy(BAD_VOLUME))), (E, "null d_colors", fix("d_colors", dev["col"]))] +
             volume_steps(pm, 0.06) + [size_step(pm)])
    walk(pm, engine, "pm_tsdf_color_clear", call, a, steps)


@gpu
def test_refusals_of_integrate_color(pm, engine, dev):
    """pm_tsdf_integrate's checks in its order, the new arguments behind them."""
    E = pm.PM_ERR_INVALID_ARG
    a = dict(camera=None, volume=None, pose=None, options=None, d_disp=None, rows=70000, cols=0, d_voxels=None, d_colors=None,
             d_bgr8=None, d_bgr=None)

    def call(lib, h, a):
        return lib.pm_tsdf_integrate_color(h, c_camera(pm, a["camera"]), c_volume(pm, a["volume"]), c_motion_ref(pm, a["pose"]),
                                           c_struct(pm.PmTsdfColorOptions, a["options"], ("min_disp", "max_range", "band")), a["d_disp"],
                                           None, a["d_bgr8"], a["d_bgr"], a["rows"], a["cols"], a["d_voxels"], a["d_colors"], None, None)

    steps = (tsdf_common_steps(pm, dev, dict(min_disp=-1.0, max_range=NAN, band=NAN)) +
             [(E, "null d_disp", fix("d_disp", dev["disp"])),
              (E, "min_disp must not be NaN or negative", fix("options", "min_disp", 0.0)),
              (E, "max_range must be >= 0 (0 = no limit)", fix("options", "max_range", 0.0))] +
             shape_steps(pm) + [size_step(pm)] +
             [(E, "null d_colors", fix("d_colors", dev["col"])),
              (E, "exactly one of d_bgr8 and d_bgr must be given (neither is)", both(fix("d_bgr8", dev["bgr8"]), fix("d_bgr", dev["bgr"]))),
              (E, "exactly one of d_bgr8 and d_bgr must be given (both are)", fix("d_bgr", None)),
              (E, "band must lie in (0, 1]", fix("options", "band", 0.0)),
              (E, "band must lie in (0, 1]", fix("options", "band", 1.5)),
              (E, "band must lie in (0, 1]", fix("options", "band", -0.5)),
              (E, "band must lie in (0, 1]", fix("options", "band", 1.0))])
    walk(pm, engine, "pm_tsdf_integrate_color", call, a, steps)


@gpu
def test_refusals_of_color_map(pm, engine, dev):
    E = pm.PM_ERR_INVALID_ARG
    a = dict(camera=None, volume=None, pose=None, options=None, d_colors=None, d_disp=None, rows=70000, cols=0, d_bgr_out=None)

    def call(lib, h, a):
        return lib.pm_tsdf_color_map(h, c_camera(pm, a["camera"]), c_volume(pm, a["volume"]), c_motion_ref(pm, a["pose"]),
                                     c_struct(pm.PmTsdfColorSampleOptions, a["options"], SAMPLE_FIELDS), a["d_colors"], a["d_disp"],
                                     a["rows"], a["cols"], a["d_bgr_out"], None, None, None)

    steps = (camera_steps(pm) +
             [(E, "null volume", fix("volume", copy.deepcopy(BAD_VOLUME))),
              (E, "null pose", fix("pose", [NAN] * 12)),
              (E, "null options", fix("options", dict(min_weight=-1.0, byte_scale=float("inf")))),
              (E, "null d_colors", fix("d_colors", dev["col"]))] +
             volume_steps(pm, 0.06) + motion_steps(pm, ("pose",), "the pose") +
             [(E, "null d_disp", fix("d_disp", dev["disp"]))] + sample_steps(pm) + shape_steps(pm) +
             [(E, "no output: d_bgr_out, d_bgr8_out, d_counts and counts are all null", fix("d_bgr_out", dev["out"])), size_step(pm)])
    walk(pm, engine, "pm_tsdf_color_map", call, a, steps)


@gpu
def test_refusals_of_color_points(pm, engine, dev):
    E = pm.PM_ERR_INVALID_ARG
    a = dict(volume=None, options=None, d_colors=None, d_xyz=None, n=-1, d_bgr_out=None)

    def call(lib, h, a):
        return lib.pm_tsdf_color_points(h, c_volume(pm, a["volume"]), c_struct(pm.PmTsdfColorSampleOptions, a["options"], SAMPLE_FIELDS),
                                        a["d_colors"], a["d_xyz"], a["n"], None, a["d_bgr_out"], None, None, None)

    steps = ([(E, "null volume", fix("volume", copy.deepcopy(BAD_VOLUME))),
              (E, "null options", fix("options", dict(min_weight=-1.0, byte_scale=float("inf")))),
              (E, "null d_colors", fix("d_colors", dev["col"])),
              (E, "null d_xyz", fix("d_xyz", dev["xyz"]))] +
             volume_steps(pm, 0.06) + sample_steps(pm) +
             [(E, "n -1 must be >= 0", fix("n", (2 ** 31 - 1) // 3 + 1)),
              (E, "no output: d_bgr_out, d_bgr8_out, d_counts and counts are all null", fix("d_bgr_out", dev["out"])),
              (pm.PM_ERR_SIZE, "n 715827883 exceeds (2^31 - 1) / 3 points", fix("n", 8)),
              size_step(pm)])
    walk(pm, engine, "pm_tsdf_color_points", call, a, steps)


@gpu
def test_nothing_is_enqueued_by_a_refusal_and_n_of_zero_only_zeroes_the_count(pm, engine):
    import torch
    grid = TR.make_grid(8, 6, 5, (-0.07, -0.05, 0.9), 0.02, 0.06, 64.0)
    cam = (40.0, 40.0, 12.0, 8.0, 0.1)
    rows, cols = 16, 24
    disp = torch.full((rows, cols), 4.25, dtype=torch.float32, device="cuda")
    image = torch.full((rows, cols, 3), 77, dtype=torch.uint8, device="cuda")
    bufs = {k: FT.Guarded(torch, n) for k, n in (("vol", 8 * 240), ("col", 16 * 240), ("out", 12 * rows * cols), ("c", 12))}
    torch.cuda.synchronize()
    for band in (float("nan"), 0.0, 1.0001):
        with pytest.raises(pm.PmError, match="band"):
            engine.tsdf_integrate_color(cam, grid, IDENT, disp.data_ptr(), rows, cols, bufs["vol"].ptr, bufs["col"].ptr,
                                        d_bgr8=image.data_ptr(), band=band, d_counts=bufs["c"].ptr)
    with pytest.raises(pm.PmError, match="exactly one"):
        engine.tsdf_integrate_color(cam, grid, IDENT, disp.data_ptr(), rows, cols, bufs["vol"].ptr, bufs["col"].ptr, d_counts=bufs["c"].ptr)
    with pytest.raises(pm.PmError, match="byte_scale"):
        engine.tsdf_color_map(cam, grid, IDENT, bufs["col"].ptr, disp.data_ptr(), rows, cols, byte_scale=-1.0, d_bgr_out=bufs["out"].ptr)
    with pytest.raises(pm.PmError, match="n -3"):
        engine.tsdf_color_points(grid, bufs["col"].ptr, bufs["out"].ptr, -3, d_bgr_out=bufs["out"].ptr)
    engine.synchronize()
    for buf in bufs.values():
        buf.read(np.uint8, 0)  # the guards and every payload byte still hold the fill
    # and the same arguments made good do run; n == 0 is legal and only zeroes the count
    engine.tsdf_clear(grid, bufs["vol"].ptr)
    engine.tsdf_color_clear(grid, bufs["col"].ptr)
    n = engine.tsdf_integrate_color(cam, grid, IDENT, disp.data_ptr(), rows, cols, bufs["vol"].ptr, bufs["col"].ptr,
                                    d_bgr8=image.data_ptr(), want_counts=True)
    assert n[0] == 240 and n[1] == 240 and 0 < n[2] <= 240
    assert engine.tsdf_color_points(grid, bufs["col"].ptr, bufs["out"].ptr, 0, d_counts=bufs["c"].ptr, want_counts=True) == 0
    engine.synchronize()
    assert bufs["c"].read(np.int32, 4)[0] == 0
    col = bufs["col"].read(np.float32).reshape(-1, 4)
    assert ((col[:, 3] == 1) == (col[:, 0] == 77)).all() and (col[:, 3] == 1).sum() == n[2]


@gpu
def test_colour_scratch_is_the_counts_the_handle_already_owns(pm):
    """The colour calls use the ONE handle-owned 16-byte allocation of the counts that pm_tsdf_integrate and pm_tsdf_raycast
    share: made on first use by whichever comes first, gone with the handle; both volumes are the caller's."""
    import torch
    lib = pm.load()
    live = lambda: (lib.pm_debug_live_device_allocations(), lib.pm_debug_live_device_bytes())
    before = live()
    grid = case_grid("37x21x13")
    cam = case_camera("37x53", True)
    vol = torch.zeros(2 * 10101, dtype=torch.float32, device="cuda")
    col = torch.zeros(4 * 10101, dtype=torch.float32, device="cuda")
    d = torch.full((37, 53), float(cam[0] * cam[4] / 1.12), dtype=torch.float32, device="cuda")
    image = torch.full((37, 53, 3), 0.5, dtype=torch.float32, device="cuda")
    out = torch.zeros((37, 53, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        base = live()
        e.tsdf_color_clear(grid, col.data_ptr())
        assert live() == base
        n = e.tsdf_integrate_color(cam, grid, IDENT, d.data_ptr(), 37, 53, vol.data_ptr(), col.data_ptr(), d_bgr=image.data_ptr(), want_counts=True)
        assert n[0] == 10101 and 0 < n[2] <= n[1] < n[0] and live() == (base[0] + 1, base[1] + 16)
        assert e.tsdf_color_map(cam, grid, IDENT, col.data_ptr(), d.data_ptr(), 37, 53, byte_scale=255.0, d_bgr8_out=out.data_ptr(), want_counts=True) > 0
        assert e.tsdf_color_points(grid, col.data_ptr(), vol.data_ptr(), 100, want_counts=True) >= 0  # any 300 floats as positions
        assert e.tsdf_integrate(cam, grid, IDENT, d.data_ptr(), 37, 53, vol.data_ptr(), want_counts=True)[0] == 10101
        assert live() == (base[0] + 1, base[1] + 16)
    assert live() == before
    got = out.cpu().numpy()
    assert set(np.unique(got)) == {0, 128}  # rintf(0.5 * 255) = rintf(127.5) = 128, half to even
