"""Undistortion + rectification of interleaved 8-bit BGR images in front of the colour Match path
(include/pm/imaging.h: pm_rectify_bgr8, pm_match_raw_bgr_device).

CPU tests pin the definition (tests/rectify_bgr_ref.py: the gray definition channel by channel at the same Q5
coordinates, one border value, one mask, the float image = byte x (float)(1 / 255.)) and run the kernel's own per-thread
code (csrc/pm_rectify.hpp: rectify_four) on the host under ASan / UBSan.  GPU tests hold the kernel to the definition
with tolerance 0 on pixels, float image and mask: the geometry is the gray kernel's (binary64, one rounding per operation,
-ffp-contract=off), the interpolation is integer, the float image is one binary32 multiplication."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rectify_bgr_ref as RB
import rectify_ref as RR
from conftest import GOLDEN, ROOT
from cpp_build import build_host_kernel
from test_rectify import _match_pair, image, radtan_view, rot

FIXTURE = os.path.join(GOLDEN, "rectify_bgr_41x59.npz")


def bgr_image(rows, cols, seed, n=None):
    """Three different channels: test_rectify.image with three seeds."""
    return np.stack([image(rows, cols, seed * 3 + c, n) for c in range(3)], axis=-1)


# ---- 1. the definition ------------------------------------------------------------------------------------------------
def test_definition_by_hand():
    """One pixel at ix = 32 * 1 + 8, iy = 32 * 2 + 24 -> weights 24*8, 8*8, 24*24, 8*24 over 1024, per channel; on the
    last column with ax = 1 the right taps read the border in every channel and the pixel is not valid."""
    g = np.arange(20, dtype=np.uint8).reshape(4, 5)
    src = np.stack([g * 10, g * 3 + 7, 250 - g * 9], axis=-1).astype(np.uint8)
    out, valid = RB.remap_bgr(src, np.array([[[40, 88]]], np.int32), 0)
    for c in range(3):
        p = src[:, :, c].astype(int)
        total = 24 * 8 * p[2, 1] + 8 * 8 * p[2, 2] + 24 * 24 * p[3, 1] + 8 * 24 * p[3, 2]
        assert out[0, 0, c] == (total + 512) >> 10
    assert valid[0, 0] == 255
    out, valid = RB.remap_bgr(src, np.array([[[4 * 32, 32], [4 * 32 + 1, 32], [-64, 0]]], np.int32), 255)
    assert np.array_equal(out[0, 0], src[1, 4]) and valid.tolist() == [[255, 0, 0]]
    for c in range(3):
        assert out[0, 1, c] == (31 * 32 * int(src[1, 4, c]) + 1 * 32 * 255 + 512) >> 10
    assert out[0, 2].tolist() == [255, 255, 255]  # every tap outside: the border in all three channels
    # the float image: one binary32 multiplication by (float)(1 / 255.), not a division
    f = RB.to_float(np.arange(256, dtype=np.uint8))
    assert f.dtype == np.float32 and f[0] == 0.0 and f[255] == np.float32(255.0) * np.float32(1.0 / 255.0)
    assert np.array_equal(f, np.arange(256, dtype=np.float32) * np.float32(0.00392156862745098))
    assert (f != np.arange(256, dtype=np.float32) / np.float32(255.0)).any()


@pytest.mark.parametrize("border", [0, 200])
def test_equal_channels_give_the_gray_definition_in_every_channel(border):
    g = image(41, 59, 2)
    view = radtan_view(41, 59, 37, 53)
    want, want_valid, want_xy = RR.rectify(g, view, 37, 53, border)
    out, out_f, valid, xy = RB.rectify_bgr(np.stack([g, g, g], axis=-1), view, 37, 53, border)
    for c in range(3):
        assert np.array_equal(out[:, :, c], want)
    assert np.array_equal(valid, want_valid) and np.array_equal(xy, want_xy)
    assert 0 < (valid == 0).mean() < 0.9
    assert np.array_equal(out_f, out.astype(np.float32) * np.float32(1.0 / 255.0))
    # n images at once: image by image
    src = bgr_image(41, 59, 5, 3)
    out, _, valid, _ = RB.rectify_bgr(src, view, 37, 53, border)
    for z in range(3):
        for c in range(3):
            assert np.array_equal(out[z, :, :, c], RR.rectify(src[z, :, :, c], view, 37, 53, border)[0])
        assert np.array_equal(valid[z], want_valid)


def test_definition_reproduces_its_fixture():
    f = np.load(FIXTURE)
    assert f["src"].shape == (41, 59, 3) and f["out"].shape == (37, 53, 3) and f["valid"].shape == (37, 53)
    out, _, valid, _ = RB.rectify_bgr(f["src"], f["view"], 37, 53, int(f["border_value"]))
    assert np.array_equal(out, f["out"]) and np.array_equal(valid, f["valid"])
    assert 0.02 < (f["valid"] == 0).mean() < 0.9  # border pixels and interior pixels
    assert not np.array_equal(f["out"][:, :, 0], f["out"][:, :, 1])  # the channels differ


# ---- 2. the kernel's own per-thread code, run on the host ----------------------------------------------------------------
@pytest.fixture(scope="module")
def host_kernel_exe(tmp_path_factory):
    """tests/cpp/rectify_host_main.cpp (the program of tests/test_rectify.py, run here in its bgr mode): csrc/pm_rectify.hpp
    compiled for the host alone, with the sanitizers."""
    return build_host_kernel(tmp_path_factory.mktemp("rectifybgrhost") / "rectify_bgr_host_main", "rectify_host_main.cpp")


def test_kernel_code_on_the_host_equals_the_definition(host_kernel_exe, tmp_path):
    """rectify_four<Bgr> and <BgrFloat> -- what every thread of k_rectify runs for BGR -- over whole images on the CPU:
    pixels, float image and mask equal the definition with tolerance 0 and the 0xA5 guards around them are intact.  The
    sources are exactly sized heap allocations (packed ones included, where the last row ends with the allocation), so AddressSanitizer
    reports a 4- or 2-byte load that reaches past byte 3 * src_cols of the last row.  The fixed shapes of the device tests
    (odd strided, odd packed, behind-camera, tiny, 64x96 radtan and identity, 1x1), three one-column sources (the path without a 6-byte window)
    and a two-column one (exactly one window), plus 40 random cases of at most 48x64 from the fuzzer's generator (seed 22)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fuzz_rectify import random_view
    rng = np.random.default_rng(22)
    # n, src_rows, src_cols, src_step, rows, cols, border, shift, outputs (1: 8 bit, 2: float, 4: mask), view
    cases = [(3, 41, 59, 192, 37, 53, 200, 1, 7, radtan_view(41, 59, 37, 53)),
             (1, 41, 59, 177, 37, 53, 0, 0, 7, radtan_view(41, 59, 37, 53)),
             (1, 41, 59, 192, 37, 53, 0, 0, 5, radtan_view(41, 59, 37, 53, R=rot(1, 100.0))),
             (1, 3, 3, 9, 8, 5, 200, 0, 3, radtan_view(3, 3, 8, 5)),
             (1, 64, 96, 288, 64, 96, 0, 0, 7, radtan_view(64, 96, 64, 96)),
             # identity: the last pixel of the last row has one tap inside, and the allocation ends with it
             (1, 64, 96, 288, 64, 96, 200, 0, 7, RR.identity_view(115.2, 115.2, 48.0, 32.0)),
             (1, 1, 1, 3, 1, 1, 9, 0, 7, RR.identity_view(1.0, 1.0, 0.0, 0.0)),
             (2, 7, 1, 3, 9, 6, 50, 2, 7, RR.identity_view(3.0, 3.0, 0.25, 3.5)),
             (1, 5, 1, 4, 6, 7, 0, 3, 6, RR.make_view([2.0, 2.0, 0.0, 2.0, 0, 0, 0, 0, 0], np.eye(3), [9.0, 2.0, 3.0, 2.5])),
             (1, 6, 2, 6, 5, 9, 77, 1, 7, RR.make_view([4.0, 4.0, 0.5, 3.0, 0, 0, 0, 0, 0], np.eye(3), [9.0, 4.0, 4.0, 2.5]))]
    for _ in range(40):
        sr, sc, rows, cols = (int(rng.integers(1, 49)), int(rng.integers(1, 65)), int(rng.integers(1, 49)),
                              int(rng.integers(1, 65)))
        cases.append((int(rng.choice([1, 2, 3])), sr, sc, 3 * sc + int(rng.choice([0, 0, 1, 5])), rows, cols,
                      int(rng.integers(0, 256)), int(rng.integers(0, 4)), int(rng.integers(1, 8)),
                      random_view(rng, sr, sc, rows, cols)[1]))
    cases = [c if c[8] & 3 else c[:8] + (c[8] | 1,) + c[9:] for c in cases]  # at least one image output
    raws = []
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for n, sr, sc, step, rows, cols, border, shift, outs, view in cases:
            raws.append(rng.integers(0, 256, (n, sr, step), dtype=np.uint8))
            f.write(np.array([n, sr, sc, step, rows, cols, border, shift, outs], np.int32).tobytes())
            f.write(np.asarray(view, np.float64).tobytes())
            f.write(raws[-1].tobytes())
    r = subprocess.run([host_kernel_exe, "bgr", str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    buf, pos = np.fromfile(tmp_path / "out.bin", np.uint8), 0
    some_valid = some_border = 0
    for (n, sr, sc, step, rows, cols, border, shift, outs, view), raw in zip(cases, raws):
        total = n * rows * cols
        dst = buf[pos:pos + 3 * total + 8]
        flt = buf[pos + 3 * total + 8:pos + 15 * total + 40]
        val = buf[pos + 15 * total + 40:pos + 16 * total + 48]
        pos += 16 * total + 48
        src = raw[:, :, :3 * sc].reshape(n, sr, sc, 3)
        want, want_f, want_valid, _ = RB.rectify_bgr(src, view, rows, cols, border)
        some_valid += int((want_valid == 255).sum())
        some_border += int((want_valid == 0).sum())
        what = (n, sr, sc, step, rows, cols, border, shift, outs)
        for bit, got, w, scale in ((1, dst, want, 1), (2, flt, want_f.view(np.uint8), 4), (4, val, want_valid, 1)):
            lo, hi = shift * scale, shift * scale + w.size
            if outs & bit:
                assert np.array_equal(got[lo:hi], w.ravel()), what + (bit,)
                assert (got[:lo] == 0xA5).all() and (got[hi:] == 0xA5).all(), what + (bit,)
            else:
                assert (got == 0xA5).all(), what + (bit,)
    assert pos == buf.size and some_valid > 1000 and some_border > 1000


# ---- 3. device parity ----------------------------------------------------------------------------------------------------
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


# name: src rows, src cols, src_step (bytes), rows, cols, n, border, view, dst offset (bytes), caller stream
DEVICE_CASES = {
    "odd_strided": (41, 59, 192, 37, 53, 1, 0, "radtan", 0, False),
    "odd_strided_border200": (41, 59, 192, 37, 53, 1, 200, "radtan", 0, False),
    "odd_strided_n3": (41, 59, 192, 37, 53, 3, 0, "radtan", 0, False),
    "odd_strided_n3_border200": (41, 59, 192, 37, 53, 3, 200, "radtan", 0, False),
    "odd_behind": (41, 59, 0, 37, 53, 1, 200, "behind", 0, False),
    "64x96_identity": (64, 96, 0, 64, 96, 1, 200, "identity", 0, False),
    "64x96_radtan": (64, 96, 0, 64, 96, 1, 0, "radtan", 0, False),
    "tiny_all_border": (3, 3, 0, 8, 5, 1, 200, "radtan", 0, False),
    "one_by_one": (1, 1, 0, 1, 1, 1, 9, "identity", 0, False),
    "unaligned_dst": (64, 96, 0, 64, 96, 1, 0, "radtan", 1, False),
    "unaligned_dst_odd_n3": (41, 59, 192, 37, 53, 3, 200, "radtan", 1, False),
    "caller_stream": (64, 96, 0, 64, 96, 3, 200, "radtan", 0, True),
    "caller_stream_odd": (41, 59, 192, 37, 53, 1, 0, "radtan", 0, True),
}
_wanted = {}


def _case(name):
    """Inputs and the definition's outputs of a device case, computed once."""
    if name not in _wanted:
        sr, sc, step, rows, cols, n, border, kind, _, _ = DEVICE_CASES[name]
        pitch = step if step else 3 * sc
        raw = np.random.default_rng(sr * 7 + cols).integers(0, 256, (n, sr, pitch), dtype=np.uint8)
        raw[:, :, :3 * sc] = bgr_image(sr, sc, cols + n, n).reshape(n, sr, 3 * sc)
        view = _view(kind, sr, sc, rows, cols)
        _wanted[name] = (raw, view) + RB.rectify_bgr(raw[:, :, :3 * sc].reshape(n, sr, sc, 3), view, rows, cols, border)[:3]
    return _wanted[name]


def _guarded(total_bytes, dtype_bytes=1):
    import torch
    return torch.full((total_bytes + 8 * dtype_bytes,), 0xA5, dtype=torch.uint8, device="cuda")


def _check(got, offset, want, what):
    inner = got[offset:offset + want.size]
    assert np.array_equal(inner, want.ravel()), "%s: %d of %d bytes differ" % (what, int((inner != want.ravel()).sum()), want.size)
    assert (got[:offset] == 0xA5).all() and (got[offset + want.size:] == 0xA5).all(), what + ": written outside the image"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DEVICE_CASES))
def test_device_pixels_float_image_and_mask_equal_the_definition(pm, engine, name):
    import torch
    sr, sc, step, rows, cols, n, border, kind, offset, own_stream = DEVICE_CASES[name]
    raw, view, want, want_f, want_valid = _case(name)
    if kind == "radtan" and sr > 8:
        assert 0 < (want_valid == 0).mean() < 0.9  # border and interior both present
    if kind == "behind":
        assert (want_valid == 0).all() and (want == border).all()
    total = n * rows * cols
    d_src = _dev(raw)
    d_dst, d_flt, d_val = _guarded(3 * total), _guarded(12 * total, 4), _guarded(total)
    torch.cuda.synchronize()
    side = torch.cuda.Stream() if own_stream else None
    stream = side.cuda_stream if side else None
    wait = side.synchronize if side else engine.synchronize
    # the 8-bit image and the mask start `offset` bytes into their allocations, the float image 4 * offset
    ptrs = (d_dst.data_ptr() + offset, d_flt.data_ptr() + 4 * offset, d_val.data_ptr() + offset)
    engine.rectify_bgr8(view, d_src.data_ptr(), n, sr, sc, step, rows, cols, border, *ptrs, stream)
    wait()
    _check(d_dst.cpu().numpy(), offset, want, "pixels")
    _check(d_flt.cpu().numpy(), 4 * offset, want_f.view(np.uint8), "float image")
    _check(d_val.cpu().numpy(), offset, want_valid, "mask")
    # each of the three outputs NULL in turn: the other two as before, the one left out untouched
    wants = ((d_dst, offset, want, "pixels"), (d_flt, 4 * offset, want_f.view(np.uint8), "float image"),
             (d_val, offset, want_valid, "mask"))
    for skip in range(3):
        for t in (d_dst, d_flt, d_val):
            t.fill_(0xA5)
        torch.cuda.synchronize()
        engine.rectify_bgr8(view, d_src.data_ptr(), n, sr, sc, step, rows, cols, border,
                            *[None if k == skip else p for k, p in enumerate(ptrs)], stream)
        wait()
        for k, (t, off, w, what) in enumerate(wants):
            if k == skip:
                assert (t.cpu().numpy() == 0xA5).all(), what + " written although NULL was passed"
            else:
                _check(t.cpu().numpy(), off, w, what + " (output %d NULL)" % skip)
    # both image outputs NULL: refused, nothing written
    with pytest.raises(pm.PmError) as err:
        engine.rectify_bgr8(view, d_src.data_ptr(), n, sr, sc, step, rows, cols, border, None, None, ptrs[2], stream)
    assert err.value.status == pm.PM_ERR_INVALID_ARG and "pm_rectify_bgr8" in str(err.value)
    wait()
    assert (d_val.cpu().numpy() == 0xA5).all()  # the mask was not written either (0xA5 since the last round above)


@pytest.mark.gpu
def test_device_reproduces_the_fixture(engine):
    import torch
    f = np.load(FIXTURE)
    d_src = _dev(f["src"])
    d_dst = torch.empty((37, 53, 3), dtype=torch.uint8, device="cuda")
    d_val = torch.empty((37, 53), dtype=torch.uint8, device="cuda")
    engine.rectify_bgr8(f["view"], d_src.data_ptr(), 1, 41, 59, 0, 37, 53, int(f["border_value"]), d_dst.data_ptr(), None,
                        d_val.data_ptr())
    engine.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), f["out"]) and np.array_equal(d_val.cpu().numpy(), f["valid"])


def _bgr_pair(synth):
    p, vl, vr = _match_pair(synth)
    return p, synth.to_bgr(p["left"], 3), synth.to_bgr(p["right"], 7), vl, vr


MATCH_MODES = {
    "scalar_seeded": dict(sem=0, kw=dict(patch=5, patchmatch_iters=2), seeded=True),
    # max_disp 40: with the default 128 the seeder's search stripe is wider than a 96-pixel image and it finds no seed
    "self_seeded": dict(sem=1, kw=dict(patch=5, patchmatch_iters=2, sparse_init=1, max_disp=40), seeded=False),
    "planes_f32": dict(sem=0, kw=dict(patch=5, patchmatch_iters=2, mode=1, state_dtype=0, max_disp=32), seeded=True),
    "planes_f16": dict(sem=0, kw=dict(patch=5, patchmatch_iters=2, mode=1, state_dtype=1, max_disp=32), seeded=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MATCH_MODES))
def test_match_raw_bgr_equals_rectify_then_match_bgr(pm, synth, mode):
    """pm_match_raw_bgr_device == pm_rectify_bgr8 x 2 + pm_match_bgr_device, torch.equal; twice into the handle's scratch
    (reused), then with the optional outputs, which receive the definition's rectified images."""
    import torch
    assert pm.PM_SEM_CPU == 0 and pm.PM_MODE_PLANES == 1 and pm.PM_STATE_F16 == 1  # the numbers MATCH_MODES uses
    m = MATCH_MODES[mode]
    rows, cols = 64, 96
    p, bl, br, vl, vr = _bgr_pair(synth)
    with pm.Engine(pm.default_params(m["sem"], **m["kw"]), max_rows=rows, max_cols=cols) as e:
        L, R = _dev(bl), _dev(br)
        SL, SR = _dev(p["seed_l"]), _dev(p["seed_r"])
        sl, sr = (SL.data_ptr(), SR.data_ptr()) if m["seeded"] else (None, None)
        RL, RRt = torch.empty_like(L), torch.empty_like(R)
        KL, KR = torch.zeros_like(L), torch.zeros_like(R)
        out = [torch.full((rows, cols), -7.0, device="cuda") for _ in range(10)]
        o = [t.data_ptr() for t in out]
        torch.cuda.synchronize()
        e.rectify_bgr8(vl, L.data_ptr(), 1, rows, cols, 0, rows, cols, 0, RL.data_ptr())
        e.rectify_bgr8(vr, R.data_ptr(), 1, rows, cols, 0, rows, cols, 0, RRt.data_ptr())
        e.match_bgr_device(1, RL.data_ptr(), RRt.data_ptr(), rows, cols, sl, sr, o[0], o[1])
        raw = (1, vl, vr, L.data_ptr(), R.data_ptr(), rows, cols, 0, rows, cols, sl, sr)
        e.match_raw_bgr_device(*raw, o[2], o[3])
        e.match_raw_bgr_device(*raw, o[4], o[5])  # again: the scratch is reused
        e.match_raw_bgr_device(*raw, o[6], o[7], KL.data_ptr(), KR.data_ptr())
        e.match_raw_bgr_device(*raw, o[8], o[9], KL.data_ptr(), None)  # one kept, one in the scratch
        e.synchronize()
        for k in (2, 4, 6, 8):
            assert torch.equal(out[k], out[0]) and torch.equal(out[k + 1], out[1]), k
        assert torch.equal(KL, RL) and torch.equal(KR, RRt)
        assert np.array_equal(KL.cpu().numpy(), RB.rectify_bgr(bl, vl, rows, cols)[0])
        assert np.array_equal(KR.cpu().numpy(), RB.rectify_bgr(br, vr, rows, cols)[0])
        got = out[0].cpu().numpy()
    assert not (got == -7.0).all() and len(np.unique(got)) > 10  # the maps are not constant


@pytest.mark.gpu
def test_match_raw_bgr_with_identity_views_equals_match_bgr_device(pm, synth):
    import torch
    rows, cols = 64, 96
    p, bl, br, _, _ = _bgr_pair(synth)
    ident = RR.identity_view(100.0, 100.0, 48.0, 32.0)
    with pm.Engine(pm.default_params(0, patch=5, patchmatch_iters=2), max_rows=rows, max_cols=cols) as e:
        L, R = _dev(bl), _dev(br)
        SL, SR = _dev(p["seed_l"]), _dev(p["seed_r"])
        out = [torch.empty((rows, cols), device="cuda") for _ in range(4)]
        e.match_bgr_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), out[0].data_ptr(),
                           out[1].data_ptr())
        e.match_raw_bgr_device(1, ident, ident, L.data_ptr(), R.data_ptr(), rows, cols, 0, rows, cols, SL.data_ptr(),
                               SR.data_ptr(), out[2].data_ptr(), out[3].data_ptr())
        e.synchronize()
        assert torch.equal(out[2], out[0]) and torch.equal(out[3], out[1])
        assert len(np.unique(out[0].cpu().numpy())) > 10


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing(pm, engine):
    import torch
    sr, sc, rows, cols = 41, 59, 37, 53
    view = radtan_view(sr, sc, rows, cols)
    src = bgr_image(sr, sc, 8)
    d_src = _dev(src)
    d_dst = torch.full((rows * cols * 3,), 0x5A, dtype=torch.uint8, device="cuda")
    d_flt = torch.full((rows * cols * 3,), -7.0, device="cuda")
    d_val = torch.full((rows * cols,), 0x5A, dtype=torch.uint8, device="cuda")
    d_keep = torch.full((2, rows * cols * 3), 0x5A, dtype=torch.uint8, device="cuda")
    d_disp = torch.full((2, rows, cols), -7.0, device="cuda")
    torch.cuda.synchronize()

    def changed(entry, value):
        v = view.copy()
        v[entry] = value
        return v

    ok = dict(view=view, d_src=d_src.data_ptr(), n=1, src_rows=sr, src_cols=sc, src_step=0, rows=rows, cols=cols,
              border_value=0, d_dst=d_dst.data_ptr(), d_dst_f=d_flt.data_ptr(), d_valid=d_val.data_ptr())
    bad_views = [None] + [changed(i, x) for i in (0, 5, 9, 17, 18, 21) for x in (np.nan, np.inf, -np.inf)] + \
                [changed(18, 0.0), changed(19, -0.0)]
    bad = [dict(view=v) for v in bad_views] + [dict(d_src=None), dict(d_dst=None, d_dst_f=None), dict(rows=0), dict(cols=0),
                                               dict(rows=-3), dict(border_value=-1), dict(border_value=256), dict(n=0),
                                               dict(src_rows=0), dict(src_cols=0), dict(src_step=3 * sc - 1),
                                               dict(src_step=sc)]
    for change in bad:
        with pytest.raises(pm.PmError) as err:
            engine.rectify_bgr8(**dict(ok, **change))
        assert err.value.status == pm.PM_ERR_INVALID_ARG and "pm_rectify_bgr8" in str(err.value), change
    with pytest.raises(pm.PmError) as err:
        engine.rectify_bgr8(**dict(ok, rows=4 * 65536))  # the launch grid's limit, as for pm_rectify_u8
    assert err.value.status == pm.PM_ERR_SIZE
    raw_ok = dict(n=1, left_view=view, right_view=view, d_left_raw=d_src.data_ptr(), d_right_raw=d_src.data_ptr(),
                  src_rows=sr, src_cols=sc, src_step=0, rows=rows, cols=cols, d_seed_l=None, d_seed_r=None,
                  d_disp_l=d_disp[0].data_ptr(), d_disp_r=d_disp[1].data_ptr(), d_left_rect=d_keep[0].data_ptr(),
                  d_right_rect=d_keep[1].data_ptr())
    E, S = pm.PM_ERR_INVALID_ARG, pm.PM_ERR_SIZE
    raw_bad = [(dict(left_view=None), E), (dict(right_view=changed(3, np.nan)), E), (dict(left_view=changed(18, 0.0)), E),
               (dict(d_left_raw=None), E), (dict(d_right_raw=None), E), (dict(d_disp_l=None), E), (dict(rows=0), E),
               (dict(cols=0), E), (dict(src_step=3 * sc - 1), E), (dict(n=0), E), (dict(rows=7), E), (dict(cols=7), E),
               (dict(rows=7, cols=7, d_left_rect=None), E), (dict(rows=65), S), (dict(cols=97), S),
               (dict(rows=4000, cols=4000), S), (dict(cols=97, d_left_rect=None, d_right_rect=None), S)]
    for change, status in raw_bad:
        with pytest.raises(pm.PmError) as err:
            engine.match_raw_bgr_device(**dict(raw_ok, **change))
        assert err.value.status == status and "pm_match_raw_bgr_device" in str(err.value), change
    engine.synchronize()
    assert (d_dst.cpu().numpy() == 0x5A).all() and (d_val.cpu().numpy() == 0x5A).all() and (d_flt.cpu().numpy() == -7.0).all()
    assert (d_keep.cpu().numpy() == 0x5A).all() and (d_disp.cpu().numpy() == -7.0).all()
    # the handle is still usable
    engine.rectify_bgr8(**ok)
    engine.synchronize()
    want, want_f, want_valid, _ = RB.rectify_bgr(src, view, rows, cols)
    assert np.array_equal(d_dst.cpu().numpy().reshape(rows, cols, 3), want)
    assert np.array_equal(d_flt.cpu().numpy().reshape(rows, cols, 3), want_f)
    assert np.array_equal(d_val.cpu().numpy().reshape(rows, cols), want_valid)


@pytest.mark.gpu
def test_differential_fuzz_of_the_bgr_rectification():
    """tools/fuzz_rectify.py --bgr, seed 12, 20 cases of at most 96x128: random sizes, strides, image counts, borders,
    alignments, streams, output subsets and views; pixels / float image / mask == tests/rectify_bgr_ref.py bit for bit."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_rectify.py"), "--bgr", "--cases", "20", "--seed", "12",
                        "--max-rows", "96", "--max-cols", "128"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
