"""Row f-3 of SURVEY.md section 8: disparity -> range -> range-dependent correction (include/pm/imaging.h).

The oracle (oracle/pm_imaging_oracle.c) restates StereoCamera::DispToDepth, imaging::RemoveBackscatter,
imaging::CorrectAttenuation, ComputeIntensity and imaging::FindDarkFast; the reference holds no expected outputs
for them (parity unpinned).  Integer / comparison results are checked exactly; float images to RTOL relative
(the device's expf and glibc's differ by at most a couple of ulp, amplified by the nested exponentials)."""
import numpy as np
import pytest

import oracle_lib as O

RTOL, ATOL = 1e-5, 1e-6

# the initial guesses of EnhanceUnderwater (src/vehicle/imaging/enhance.cpp:44-49) and a beta_D of the same scale
B0 = (0.132, 0.115, 0.0559)
BETA_B0 = (0.358, 0.695, 1.11)
X0 = (0.30, 0.25, 0.40, -0.20, -0.15, -0.30, 0.10, 0.12, 0.08, -0.05, -0.04, -0.06)


def scene(rows, cols, seed):
    rng = np.random.default_rng(seed)
    disp = rng.uniform(2.0, 96.0, (rows, cols)).astype(np.float32)
    disp[rng.random((rows, cols)) < 0.2] = 0.0  # masked-out pixels: no range
    bgr = rng.uniform(0.0, 1.0, (rows, cols, 3)).astype(np.float32)
    return bgr, disp


# ---- oracle known answers (CPU) ------------------------------------------------------------------------
def test_oracle_disp_to_range_known_values():
    d = np.array([[0.0, -1.0, 1.0, 2.0, 50.0, 0.5]], np.float32)
    r = O.disp_to_range(d, 400.0, 0.25)
    assert r.tolist() == [[0.0, 0.0, 100.0, 50.0, 2.0, 200.0]]
    # double division, then one rounding to float
    d = np.array([[3.0, 7.0]], np.float32)
    assert r.dtype == np.float32 and np.array_equal(O.disp_to_range(d, 415.876509, 0.12),
                                                    np.float32(415.876509 * 0.12 / d.astype(np.float64)))


def test_oracle_backscatter_and_attenuation_closed_form():
    bgr = np.full((1, 3, 3), 0.5, np.float32)
    rng = np.array([[0.0, 1.0, 4.0]], np.float32)
    out = O.remove_backscatter(bgr, rng, B0, BETA_B0)
    z = np.array([20.0, 1.0, 4.0])  # no range -> 20 m of water column
    for c in range(3):
        want = np.maximum(0.5 - B0[c] * (1.0 - np.exp(-BETA_B0[c] * z)), 0.0)
        assert np.allclose(out[0, :, c], want, rtol=1e-6)
    # range 0 with B = 1 removes everything (clamped at 0)
    assert O.remove_backscatter(bgr, rng, (1, 1, 1), (5, 5, 5))[0, 0].tolist() == [0.0, 0.0, 0.0]
    out = O.correct_attenuation(bgr, rng, X0)
    z = np.array([4.0, 1.0, 4.0])  # no range -> the largest range of the map
    for c in range(3):
        beta = X0[c] * np.exp(X0[3 + c] * z) + X0[6 + c] * np.exp(X0[9 + c] * z)
        assert np.allclose(out[0, :, c], 0.5 * np.exp(beta * z), rtol=1e-6)


def test_oracle_intensity_and_find_dark():
    bgr = np.zeros((2, 2, 3), np.float32)
    bgr[0, 0] = (1, 0, 0)
    bgr[0, 1] = (0, 1, 0)
    bgr[1, 0] = (0, 0, 1)
    bgr[1, 1] = (1, 1, 1)
    g = O.compute_intensity(bgr)
    assert g[0, 0] == np.float32(0.114) and g[0, 1] == np.float32(0.587) and g[1, 0] == np.float32(0.299)
    assert abs(g[1, 1] - 1.0) < 1e-6
    # uniform intensities: the 1 % threshold over pixels with range ends near 0.01
    rng = np.random.default_rng(3)
    inten = rng.uniform(0, 1, (200, 300)).astype(np.float32)
    rmap = np.ones((200, 300), np.float32)
    thr, mask = O.find_dark(inten, rmap, 0.01)
    assert 0.008 < thr < 0.012
    assert abs(int((mask > 0).sum()) - 600) < 60
    # pixels without range never count
    rmap[:, :150] = 0.05
    thr2, mask2 = O.find_dark(inten, rmap, 0.01)
    assert thr2 > thr and not mask2[:, :150].any()


# ---- device parity ----------------------------------------------------------------------------------------
def _dev(t, a):
    return t.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(48, 64), (37, 53), (1, 7), (240, 322)])
def test_device_stages_match_oracle(pm, rows, cols):
    import torch
    bgr, disp = scene(rows, cols, rows * 7 + cols)
    fx, baseline = 415.876509, 0.12
    with pm.Engine(pm.default_params(0, patch=5), max_rows=max(rows, 16), max_cols=max(cols, 16)) as e:
        d_disp, d_bgr = _dev(torch, disp), _dev(torch, bgr)
        d_range = torch.empty_like(d_disp)
        e.disp_to_range(d_disp.data_ptr(), rows, cols, fx, baseline, d_range.data_ptr())
        e.synchronize()
        want_range = O.disp_to_range(disp, fx, baseline)
        assert np.array_equal(d_range.cpu().numpy(), want_range), "DispToDepth is exact (double divide, one rounding)"

        d_out = torch.empty_like(d_bgr)
        e.remove_backscatter(d_bgr.data_ptr(), d_range.data_ptr(), rows, cols, B0, BETA_B0, d_out.data_ptr())
        e.synchronize()
        want_d = O.remove_backscatter(bgr, want_range, B0, BETA_B0)
        np.testing.assert_allclose(d_out.cpu().numpy(), want_d, rtol=RTOL, atol=ATOL)

        d_j = torch.empty_like(d_bgr)
        e.correct_attenuation(d_out.data_ptr(), d_range.data_ptr(), rows, cols, X0, d_j.data_ptr())
        e.synchronize()
        want_j = O.correct_attenuation(want_d, want_range, X0)
        np.testing.assert_allclose(d_j.cpu().numpy(), want_j, rtol=RTOL, atol=ATOL)

        # the fused pass equals the chain
        d_f, d_r2 = torch.empty_like(d_bgr), torch.empty_like(d_disp)
        e.range_enhance(d_bgr.data_ptr(), d_disp.data_ptr(), rows, cols, fx, baseline, B0, BETA_B0, X0,
                        d_r2.data_ptr(), d_f.data_ptr())
        e.synchronize()
        assert torch.equal(d_r2, d_range)
        assert torch.equal(d_f, d_j), "fused kernel = the three stages, bit for bit on the device"

        d_g = torch.empty_like(d_disp)
        e.compute_intensity(d_bgr.data_ptr(), rows, cols, d_g.data_ptr())
        e.synchronize()
        assert np.array_equal(d_g.cpu().numpy(), O.compute_intensity(bgr)), "BGR2GRAY: three products, two sums"

        d_mask = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
        thr = e.find_dark(d_g.data_ptr(), d_range.data_ptr(), rows, cols, 0.05, d_mask.data_ptr())
        want_thr, want_mask = O.find_dark(O.compute_intensity(bgr), want_range, 0.05)
        assert thr == want_thr and np.array_equal(d_mask.cpu().numpy(), want_mask)


@pytest.mark.gpu
def test_unaligned_pointers_and_errors(pm):
    import torch
    rows, cols = 20, 33
    bgr, disp = scene(rows, cols, 5)
    with pm.Engine(pm.default_params(0, patch=5), max_rows=32, max_cols=64) as e:
        # views that start 4 bytes into an allocation: the kernels must not assume 16-byte alignment
        buf_b = torch.zeros(rows * cols * 3 + 1, device="cuda")
        buf_r = torch.zeros(rows * cols + 1, device="cuda")
        buf_o = torch.zeros(rows * cols * 3 + 1, device="cuda")
        buf_b[1:] = _dev(torch, bgr).reshape(-1)
        rng = O.disp_to_range(disp, 400.0, 0.1)
        buf_r[1:] = _dev(torch, rng).reshape(-1)
        e.remove_backscatter(buf_b[1:].data_ptr(), buf_r[1:].data_ptr(), rows, cols, B0, BETA_B0, buf_o[1:].data_ptr())
        e.synchronize()
        got = buf_o[1:].cpu().numpy().reshape(rows, cols, 3)
        np.testing.assert_allclose(got, O.remove_backscatter(bgr, rng, B0, BETA_B0), rtol=RTOL, atol=ATOL)
        with pytest.raises(pm.PmError) as err:
            e.disp_to_range(0, rows, cols, 1.0, 1.0, buf_r.data_ptr())
        assert err.value.status == pm.PM_ERR_INVALID_ARG


@pytest.mark.gpu
def test_stereo_to_corrected_image_without_host_round_trip(pm, oracle, synth):
    """Match() -> disparity -> range -> correction, all enqueued on the handle's stream."""
    import torch
    rows, cols = 96, 160
    p = synth.make_pair(3, rows, cols)
    rng = np.random.default_rng(1)
    bgr = rng.uniform(0, 1, (rows, cols, 3)).astype(np.float32)
    with pm.Engine(pm.default_params(0, patch=5, patchmatch_iters=2), max_rows=rows, max_cols=cols) as e:
        L, R = _dev(torch, p["left"]), _dev(torch, p["right"])
        SL, SR = _dev(torch, p["seed_l"]), _dev(torch, p["seed_r"])
        DL, DR = torch.empty_like(SL), torch.empty_like(SR)
        d_bgr, d_out = _dev(torch, bgr), torch.empty((rows, cols, 3), device="cuda")
        e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), DL.data_ptr(),
                       DR.data_ptr())
        e.range_enhance(d_bgr.data_ptr(), DL.data_ptr(), rows, cols, 400.0, 0.1, B0, BETA_B0, X0, None,
                        d_out.data_ptr())
        e.synchronize()
    el, _ = oracle.match(oracle.default_params(0, patch=5, n_iters=2, nthreads=8), p["left"], p["right"],
                         p["seed_l"], p["seed_r"])
    r = O.disp_to_range(el, 400.0, 0.1)
    want = O.correct_attenuation(O.remove_backscatter(bgr, r, B0, BETA_B0), r, X0)
    np.testing.assert_allclose(d_out.cpu().numpy(), want, rtol=RTOL, atol=ATOL)


# ---- edges: disparity maps, alignment, pixel counts, launch caps, FindDarkFast's paths -----------------------------
FX, BASELINE = 415.876509, 0.12  # fx * baseline = 49.9...


def _assert_close(got, want, what):
    """RTOL / ATOL of this file; NaN and inf must sit at the same positions (assert_allclose checks both)."""
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)


def _chain_and_fused(torch, e, bgr, disp, what, want=None):
    """disp -> range -> backscatter -> attenuation on the device against the oracle, and pm_range_enhance (with and
    without the range output) against the device chain bit for bit.  Returns the oracle's (range, backscatter, result)."""
    rows, cols = disp.shape
    d_disp, d_bgr = _dev(torch, disp), _dev(torch, bgr)
    d_range, d_b, d_j = torch.empty_like(d_disp), torch.empty_like(d_bgr), torch.empty_like(d_bgr)
    e.disp_to_range(d_disp.data_ptr(), rows, cols, FX, BASELINE, d_range.data_ptr())
    e.remove_backscatter(d_bgr.data_ptr(), d_range.data_ptr(), rows, cols, B0, BETA_B0, d_b.data_ptr())
    e.correct_attenuation(d_b.data_ptr(), d_range.data_ptr(), rows, cols, X0, d_j.data_ptr())
    d_f, d_f2, d_r2 = torch.empty_like(d_bgr), torch.empty_like(d_bgr), torch.empty_like(d_disp)
    e.range_enhance(d_bgr.data_ptr(), d_disp.data_ptr(), rows, cols, FX, BASELINE, B0, BETA_B0, X0, d_r2.data_ptr(),
                    d_f.data_ptr())
    e.range_enhance(d_bgr.data_ptr(), d_disp.data_ptr(), rows, cols, FX, BASELINE, B0, BETA_B0, X0, None,
                    d_f2.data_ptr())
    e.synchronize()
    if want is None:
        want_range = O.disp_to_range(disp, FX, BASELINE)
        want_b = O.remove_backscatter(bgr, want_range, B0, BETA_B0)
        want = (want_range, want_b, O.correct_attenuation(want_b, want_range, X0))
    assert np.array_equal(d_range.cpu().numpy(), want[0]), f"{what}: range map"
    _assert_close(d_b.cpu().numpy(), want[1], f"{what}: RemoveBackscatter")
    _assert_close(d_j.cpu().numpy(), want[2], f"{what}: CorrectAttenuation")
    assert torch.equal(d_r2, d_range), f"{what}: fused range map"
    j = d_j.cpu().numpy()
    assert np.array_equal(d_f.cpu().numpy(), j, equal_nan=True), f"{what}: fused = chain"
    assert np.array_equal(d_f2.cpu().numpy(), j, equal_nan=True), f"{what}: fused without range output = chain"
    return want


@pytest.mark.gpu
def test_disparity_map_edges(pm):
    import torch
    rows, cols = 5, 7  # 35 pixels: 8 float4 groups and a scalar tail of 3
    rng = np.random.default_rng(21)
    bgr = rng.uniform(0.0, 1.0, (rows, cols, 3)).astype(np.float32)
    with pm.Engine(pm.default_params(0, patch=5), max_rows=16, max_cols=16) as e:
        # all zeros: the +inf sentinel of the smallest positive disparity means rmax = 0, z = 0, exp(0) = 1
        zero = np.zeros((rows, cols), np.float32)
        want = _chain_and_fused(torch, e, bgr, zero, "all zeros")
        assert not want[0].any()
        d_bgr, d_zero, d_out = _dev(torch, bgr), _dev(torch, zero), torch.zeros((rows, cols, 3), device="cuda")
        e.correct_attenuation(d_bgr.data_ptr(), d_zero.data_ptr(), rows, cols, X0, d_out.data_ptr())
        e.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), bgr), "no range anywhere: CorrectAttenuation returns its input"
        # exactly one positive pixel: first, last of the float4 part, in the scalar tail, last
        for pos in (0, 31, 33, 34):
            d = np.zeros(rows * cols, np.float32)
            d[pos] = 7.5
            want = _chain_and_fused(torch, e, bgr, d.reshape(rows, cols), f"one positive pixel at {pos}")
            assert want[0].max() == np.float32(FX * BASELINE / 7.5)
        # special values.  inf -> range 0 (fx b / inf); a tiny normal disparity -> a huge finite largest range; a denormal
        # one -> range +inf, so every pixel without range gets z = inf and NaN out of CorrectAttenuation (inf * 0)
        tiny, denormal = np.float32(1e-30), np.float32(1e-40)
        assert 0 < denormal < np.finfo(np.float32).tiny
        base = rng.uniform(2.0, 96.0, rows * cols).astype(np.float32)
        base[[1, 6, 12, 18, 30, 32]] = [-3.0, -0.0, np.nan, np.inf, -np.inf, np.nan]
        base[[2, 34]] = [0.0, -1e-40]
        base[[9, 33]] = 1.0e5       # 0 < range <= 1e-3: background for the backscatter, a range for the attenuation
        base[[10, 20]] = [1000.0, 499.5]  # ranges in (1e-3, 0.1]
        for name, extra in (("finite", None), ("tiny normal", tiny), ("denormal", denormal)):
            d = base.copy()
            if extra is not None:
                d[[5, 33]] = extra
            want = _chain_and_fused(torch, e, bgr, d.reshape(rows, cols), f"special values, {name}")
            r = want[0].reshape(-1)
            assert not r[[1, 6, 12, 18, 30, 32, 2, 34]].any()
            assert 0 < r[9] <= 1e-3 and 1e-3 < r[10] <= 0.1 and 1e-3 < r[20] <= 0.1
            if name == "denormal":
                assert np.isinf(r[5]) and np.isnan(want[2].reshape(-1, 3)[1]).all()
            else:
                assert np.isfinite(r).all() and np.isfinite(want[2]).all()


@pytest.mark.gpu
def test_pixel_counts_around_the_float4_groups(pm):
    import torch
    rng = np.random.default_rng(22)
    with pm.Engine(pm.default_params(0, patch=5), max_rows=16, max_cols=16) as e:
        for rows, cols in [(1, 1), (1, 2), (1, 3), (2, 2), (1, 5), (2, 3), (7, 1), (2, 4), (3, 3), (1, 257), (2, 513)]:
            bgr = rng.uniform(0.0, 1.0, (rows, cols, 3)).astype(np.float32)
            disp = rng.uniform(2.0, 96.0, (rows, cols)).astype(np.float32)
            disp[rng.random((rows, cols)) < 0.3] = 0.0
            _chain_and_fused(torch, e, bgr, disp, f"{rows}x{cols}")
            disp[-1, -1] = 1.25  # the largest range in the last pixel (the scalar tail where there is one)
            _chain_and_fused(torch, e, bgr, disp, f"{rows}x{cols}, largest range last")


@pytest.mark.gpu
def test_unaligned_pointers_of_attenuation_and_fused_pass(pm):
    """Every pointer in turn starts 4 bytes into its allocation: the vec_ok = 0 paths of k_range_enhance<2> and <7> and of
    k_disp_min_positive.  Results: the oracle's to tolerance, and the aligned call's bit for bit."""
    import torch
    rows, cols = 21, 33  # 693 pixels = 173 float4 groups + 1
    n = rows * cols
    bgr, disp = scene(rows, cols, 6)
    disp.reshape(-1)[-1] = 1.5  # the smallest positive disparity in the last pixel
    rng_map = O.disp_to_range(disp, FX, BASELINE)
    want_att = O.correct_attenuation(bgr, rng_map, X0)
    want_fused = O.correct_attenuation(O.remove_backscatter(bgr, rng_map, B0, BETA_B0), rng_map, X0)

    def view(a, off):
        buf = torch.zeros(a.size + 1, device="cuda")
        v = buf[1:] if off else buf[:-1]
        v.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        assert (v.data_ptr() % 16 == 4) == bool(off)
        return v

    with pm.Engine(pm.default_params(0, patch=5), max_rows=32, max_cols=64) as e:
        results = []
        for which in (None, "bgr", "range", "out"):
            b, r = view(bgr, which == "bgr"), view(rng_map, which == "range")
            o = view(np.zeros(n * 3, np.float32), which == "out")
            e.correct_attenuation(b.data_ptr(), r.data_ptr(), rows, cols, X0, o.data_ptr())
            e.synchronize()
            results.append(o.cpu().numpy().reshape(rows, cols, 3))
            _assert_close(results[-1], want_att, f"pm_correct_attenuation, {which} unaligned")
            assert np.array_equal(results[-1], results[0]), which
        for with_range in (True, False):
            results = []
            for which in (None, "bgr", "disp", "out") + (("range_out",) if with_range else ()):
                b, d = view(bgr, which == "bgr"), view(disp, which == "disp")
                o = view(np.zeros(n * 3, np.float32), which == "out")
                ro = view(np.zeros(n, np.float32), which == "range_out") if with_range else None
                e.range_enhance(b.data_ptr(), d.data_ptr(), rows, cols, FX, BASELINE, B0, BETA_B0, X0,
                                ro.data_ptr() if with_range else None, o.data_ptr())
                e.synchronize()
                results.append(o.cpu().numpy().reshape(rows, cols, 3))
                _assert_close(results[-1], want_fused, f"pm_range_enhance, {which} unaligned")
                assert np.array_equal(results[-1], results[0]), which
                if with_range:
                    assert np.array_equal(ro.cpu().numpy().reshape(rows, cols), rng_map), which


@pytest.mark.gpu
def test_fused_pass_beyond_its_launch_cap(pm):
    """2050 x 2049 = 4 200 450 pixels: more float4 groups than the 4096 x 256 lanes of the capped grid (and than the
    2048 x 256 of the reduction's), so every grid-stride loop runs a second trip; n % 4 = 2."""
    import torch
    rows, cols = 2050, 2049
    assert rows * cols // 4 > 4 * 256 * 16 * 256 // 4 + 1 and rows * cols % 4 == 2
    bgr, disp = scene(rows, cols, 9)
    disp.reshape(-1)[-3] = 1.0  # the smallest positive disparity: met only in the second trip
    with pm.Engine(pm.default_params(0, patch=5), max_rows=16, max_cols=16) as e:
        want = _chain_and_fused(torch, e, bgr, disp, "2050x2049")
    assert want[0].max() == np.float32(FX * BASELINE) and want[0].reshape(-1)[-3] == want[0].max()


@pytest.mark.gpu
def test_streaming_stages_beyond_their_launch_caps(pm):
    """1025 x 1024 = 1 049 600 pixels: more than the 4096 x 256 lanes of the one-pixel-per-lane stages (and twice the
    2048 x 256 of the reductions k_range_max and k_dark_count)."""
    import torch
    rows, cols = 1025, 1024
    assert rows * cols > 256 * 16 * 256
    bgr, disp = scene(rows, cols, 10)
    disp.reshape(-1)[-1] = 1.0  # the largest range in the last pixel
    with pm.Engine(pm.default_params(0, patch=5), max_rows=16, max_cols=16) as e:
        d_disp, d_bgr = _dev(torch, disp), _dev(torch, bgr)
        d_range, d_g, d_j = torch.empty_like(d_disp), torch.empty_like(d_disp), torch.empty_like(d_bgr)
        d_mask = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
        e.disp_to_range(d_disp.data_ptr(), rows, cols, FX, BASELINE, d_range.data_ptr())
        e.compute_intensity(d_bgr.data_ptr(), rows, cols, d_g.data_ptr())
        e.correct_attenuation(d_bgr.data_ptr(), d_range.data_ptr(), rows, cols, X0, d_j.data_ptr())
        thr = e.find_dark(d_g.data_ptr(), d_range.data_ptr(), rows, cols, 0.05, d_mask.data_ptr())
        d_n = torch.empty_like(d_bgr)
        e.normalize(d_bgr.data_ptr(), rows, cols, d_n.data_ptr())
        e.synchronize()
        want_range = O.disp_to_range(disp, FX, BASELINE)
        assert want_range.reshape(-1)[-1] == want_range.max()
        assert np.array_equal(d_range.cpu().numpy(), want_range)
        gray = O.compute_intensity(bgr)
        assert np.array_equal(d_g.cpu().numpy(), gray)
        _assert_close(d_j.cpu().numpy(), O.correct_attenuation(bgr, want_range, X0), "CorrectAttenuation")
        want_thr, want_mask = O.find_dark(gray, want_range, 0.05)
        assert thr == want_thr and np.array_equal(d_mask.cpu().numpy(), want_mask)
        assert np.array_equal(d_n.cpu().numpy(), O.normalize(bgr)), "Normalize"


def _dark_case(name):
    """(intensity, range, percentile) of a 10x10 image, n_desired = 10 unless stated."""
    inten = np.full(100, 0.9, np.float32)
    rmap = np.ones(100, np.float32)
    p = 0.1
    if name == "first probe hits":      # 10 pixels under 1.5 * 0.1: the early return, the mask is that step's
        inten[3:13] = 0.01
    elif name == "met inside the loop":  # 15 under 0.15 -> high = 0.15; 10 under 0.075
        inten[3:13] = 0.01
        inten[50:55] = 0.14
    elif name == "nothing desired":      # (int)(0.001 * 100) = 0, yet 3 pixels are always dark: the final midpoint
        inten[[0, 57, 99]] = 0.0
        p = 0.001
    elif name == "percentile zero":      # first = 0, nothing <= 0: count 0 == n_desired 0 at once
        p = 0.0
    elif name == "no pixel with range":  # ranges in (1e-3, 0.1] and exactly 0.1f: every count is 0
        inten[3:13] = 0.01
        rmap[:] = np.linspace(0.002, 0.1, 100, dtype=np.float32)
        rmap[7] = np.float32(0.1)
    elif name == "range just above 0.1":  # only the pixels whose range exceeds 0.1f count
        inten[:20] = 0.01
        rmap[:10] = np.float32(0.1)
        rmap[10:20] = np.nextafter(np.float32(0.1), np.float32(1))
    return inten.reshape(10, 10), rmap.reshape(10, 10), p


DARK_CASES = {"first probe hits": (np.float32(1.5 * np.float32(0.1)), 10), "met inside the loop": (0.075, 10),
              "nothing desired": (None, 3), "percentile zero": (0.0, 0), "no pixel with range": (None, 0),
              "range just above 0.1": (np.float32(1.5 * np.float32(0.1)), 10)}


def test_oracle_find_dark_paths():
    for name, (thr_want, n_mask) in DARK_CASES.items():
        inten, rmap, p = _dark_case(name)
        thr, mask = O.find_dark(inten, rmap, p)
        assert int((mask > 0).sum()) == n_mask, name
        if thr_want is not None:
            assert thr == float(np.float32(thr_want)), name
    # the final midpoints: low = 0.15 pushed up 8 times towards 0.5; high = 0.0015 halved 8 times
    lo, hi = np.float32(1.5 * np.float32(0.1)), np.float32(0.5)
    for _ in range(8):
        lo = (hi + lo) / np.float32(2.0)
    assert O.find_dark(*_dark_case("no pixel with range"))[0] == float((hi + lo) / np.float32(2.0))
    assert 0 < O.find_dark(*_dark_case("nothing desired"))[0] < 0.0015 / 256


@pytest.mark.gpu
def test_find_dark_paths(pm):
    import torch
    with pm.Engine(pm.default_params(0, patch=5), max_rows=16, max_cols=16) as e:
        for name in DARK_CASES:
            inten, rmap, p = _dark_case(name)
            d_i, d_r = _dev(torch, inten), _dev(torch, rmap)
            d_mask = torch.full((10, 10), 7, dtype=torch.uint8, device="cuda")
            thr = e.find_dark(d_i.data_ptr(), d_r.data_ptr(), 10, 10, p, d_mask.data_ptr())
            want_thr, want_mask = O.find_dark(inten, rmap, p)
            assert thr == want_thr, name
            assert np.array_equal(d_mask.cpu().numpy(), want_mask), name
