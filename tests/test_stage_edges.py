"""The stages that turn a CALLER's disparity map into addresses, at their edges: pm_mask_occlusions, pm_remove_background,
pm_propagate, pm_add_noise, and the seed path of Match() with patchmatch_iters == 0 (k_seed -> background -> k_finalize).

Whole-path tests only feed these stages maps the noise step has clamped to >= 0 and that are mostly zeros.  Here the maps
are built so that the rule under test decides the pixel:
  * threshold maps: dr sits on the float next to 1.4 * dl / 0.7 * dl, so a comparison in binary32 instead of binary64
    (patchmatch_gpu.cu:273-295: double literals) gives another map;
  * truncation maps: x - dl has fractions .5, .99 and .0 and neighbouring columns of dr decide differently, so rounding
    instead of truncating the column gives another map;
  * dense RemoveBackground maps with a factor chosen (on the CPU, on the oracle) so that the threshold keeps and zeroes
    at least a quarter of the interior each, for every tiled window and the generic kernel;
  * maps whose values would index past the row are REFUSED by the entry points (include/pm/patchmatch.h); they are only
    ever given to the guards, never to a kernel.
Tolerance 0 everywhere; maps with NaN, -0.0 and infinities are compared as bit patterns.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pyref

f32 = np.float32


def assert_bits(a, b, what=""):
    """Bit-for-bit equality of float32 maps, NaN and the sign of zero included."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    if not np.array_equal(ua, ub):
        bad = np.argwhere(ua != ub)
        y, x = bad[0][:2]
        raise AssertionError(f"{what}: {len(bad)} of {a.size} values differ; first at (y={y}, x={x}): "
                             f"{a[y, x]!r} vs {b[y, x]!r}")


# ---- map families -------------------------------------------------------------------------------------------
def column_of(dl):
    """(int)fmaxf((float)x - dl, 0.f) for every pixel: binary32 subtraction, NaN -> 0, truncation."""
    xs = np.arange(dl.shape[1], dtype=np.float32)[None, :]
    with np.errstate(invalid="ignore"):
        pos = np.fmax(xs - dl.astype(np.float32), f32(0))
    return pos, pos.astype(np.int64)


def rule64(dl, dr):
    """MaskOcclusions stated in numpy: the column in binary32, the comparison in binary64."""
    dl, dr = np.asarray(dl, np.float32), np.asarray(dr, np.float32)
    _, xr = column_of(dl)
    drs = np.take_along_axis(dr, xr, axis=1).astype(np.float64)
    d = dl.astype(np.float64)
    with np.errstate(invalid="ignore"):
        zero = (drs > 1.4 * d) | (drs < 0.7 * d)
    out = dl.copy()
    out[zero] = 0
    return out


def threshold_maps(rows, cols, seed, dmax=500):
    """dl: multiples of 1/8 in (0, dmax), at most x so that the columns x - dl spread over the row; dr at the column a
    pixel reads (the first pixel to claim a column sets it): the float nearest 1.4 * dl or 0.7 * dl, or one of its two
    neighbours."""
    rng = np.random.default_rng(seed)
    dl = np.zeros((rows, cols), np.float32)
    dr = rng.uniform(0.0, float(min(dmax, max(cols, 2))), (rows, cols)).astype(np.float32)
    for y in range(rows):
        used = set()
        for x in rng.permutation(cols):
            kmax = min(8 * dmax - 1, 8 * int(x))
            k = int(rng.integers(1, kmax + 1)) if kmax >= 1 else int(rng.integers(1, 8))
            d = f32(k / 8.0)
            dl[y, x] = d
            xr = int(max(f32(f32(x) - d), f32(0)))
            if xr in used:
                continue
            used.add(xr)
            t = f32((1.4 if rng.random() < 0.5 else 0.7) * float(d))
            pick = int(rng.integers(3))
            dr[y, xr] = t if pick == 0 else np.nextafter(t, f32(np.inf if pick == 1 else -np.inf))
    return dl, dr


def float_compare_disagrees(dl, dr):
    """Pixels on which `dr > 1.4f * dl || dr < 0.7f * dl` in binary32 decides otherwise than the binary64 rule."""
    _, xr = column_of(dl)
    drs = np.take_along_axis(np.asarray(dr, np.float32), xr, axis=1)
    z32 = (drs > f32(1.4) * dl) | (drs < f32(0.7) * dl)
    d = dl.astype(np.float64)
    z64 = (drs.astype(np.float64) > 1.4 * d) | (drs.astype(np.float64) < 0.7 * d)
    return z32 != z64


def truncation_maps(rows, cols, seed):
    """x - dl with fractions .5, .99 and .0 (dl in a narrow band [b, 1.3 b], so that dl > x on the first columns: column
    0); dr alternates between a value every dl of the band accepts (even columns) and one it rejects (odd columns), so the
    neighbouring column decides otherwise.  The last columns hold dl = -m at x = cols - 1 - m: x - dl == cols - 1 exactly;
    dr(cols - 1) is NaN on every other row (NaN rejects nothing: the pixel keeps its negative value)."""
    rng = np.random.default_rng(seed)
    b = max(2, min(20, cols // 6))
    jlo, jhi = b + 1, max(b + 1, int(1.3 * b))
    j = rng.integers(jlo, jhi + 1, (rows, cols)).astype(np.float64)
    frac = rng.choice(np.array([0.5, 0.99, 0.0]), (rows, cols))
    dl = (j - frac).astype(np.float32)
    dr = np.tile(np.where(np.arange(cols) % 2 == 0, f32(1.1 * b), f32(10 * b + 100)).astype(np.float32), (rows, 1))
    for m in range(min(4, cols)):
        dl[:, cols - 1 - m] = f32(-m) if m else f32(-0.0)
    dr[1::2, cols - 1] = np.nan
    return dl, dr


def rounding_selects_otherwise(dl, dr):
    """Pixels at which rint(x - dl) and trunc(x - dl) pick different VALUES of dr."""
    pos, xr = column_of(dl)
    xn = np.clip(np.rint(pos).astype(np.int64), 0, dl.shape[1] - 1)
    a, b = np.take_along_axis(dr, xr, axis=1), np.take_along_axis(dr, xn, axis=1)
    return a.view(np.uint32) != b.view(np.uint32)


def dense_maps(rows, cols, seed):
    rng = np.random.default_rng(seed)
    hi = max(1.0, cols / 2.0)
    return (rng.uniform(0.0, hi, (rows, cols)).astype(np.float32), rng.uniform(0.0, hi, (rows, cols)).astype(np.float32))


def special_maps(rows, cols, seed):
    """A dense pair with, in dl: NaN, +inf, -0.0, a denormal, and negatives that stay in the row (x - dl <= cols - 1);
    in dr: NaN and both infinities."""
    rng = np.random.default_rng(seed)
    dl, dr = dense_maps(rows, cols, seed + 1)
    pick = rng.integers(0, 12, (rows, cols))
    xs = np.arange(cols)[None, :].repeat(rows, 0)
    room = (cols - 1 - xs).astype(np.float32)                       # the largest m with x + m <= cols - 1
    neg = -np.floor(room * rng.random((rows, cols)).astype(np.float32))
    dl = np.where(pick == 0, f32(np.nan), dl)
    dl = np.where(pick == 1, f32(np.inf), dl)
    dl = np.where(pick == 2, f32(-0.0), dl)
    dl = np.where(pick == 3, f32(1e-40), dl)
    dl = np.where(pick == 4, neg, dl).astype(np.float32)
    dl = np.where(pick == 5, -room, dl).astype(np.float32)          # x - dl == cols - 1 exactly
    pr = rng.integers(0, 10, (rows, cols))
    dr = np.where(pr == 0, f32(np.nan), dr)
    dr = np.where(pr == 1, f32(np.inf), dr)
    dr = np.where(pr == 2, f32(-np.inf), dr).astype(np.float32)
    return np.ascontiguousarray(dl), np.ascontiguousarray(dr)


FAMILIES = {"threshold": threshold_maps, "truncation": truncation_maps, "dense": dense_maps, "special": special_maps}
MO_SHAPES = [(1, 1), (1, 2), (3, 255), (2, 256), (2, 257), (5, 513)]  # the launch uses 256-lane blocks over columns


@functools.lru_cache(maxsize=None)
def mo_case(family, rows, cols):
    dl, dr = FAMILIES[family](rows, cols, 7 * rows + cols)
    dl.setflags(write=False)
    dr.setflags(write=False)
    return dl, dr


def out_of_row_maps(rows, cols):
    """(what, dl) whose column leaves the row: -1 at the last column, -inf, -cols at column 0."""
    base = np.full((rows, cols), 1.0, np.float32)
    out = []
    for what, y, x, v in (("-1 at x = cols - 1", rows - 1, cols - 1, -1.0), ("-inf", 0, cols // 2, -np.inf),
                          ("-cols at x = 0", rows - 1, 0, -float(cols))):
        m = base.copy()
        m[y, x] = v
        out.append((what, m, y * cols + x))
    return out


# ---- CPU: the oracle against two independent statements of MaskOcclusions ------------------------------------------
@pytest.mark.parametrize("family", ["threshold", "truncation", "dense", "special"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 255), (5, 513), (8, 47), (7, 257)])
def test_oracle_mask_occlusions_equals_numpy_and_pyref(oracle, family, shape):
    dl, dr = mo_case(family, *shape)
    got = oracle.gpu_mask_occlusions(dl, dr)
    assert_bits(got, rule64(dl, dr), f"{family} {shape}: oracle vs the binary64 rule in numpy")
    assert_bits(got, pyref.gpu_mask_occlusions(dl, dr), f"{family} {shape}: oracle vs pyref")


@pytest.mark.parametrize("shape", [(3, 255), (2, 256), (2, 257), (5, 513), (8, 47), (7, 257)])
def test_threshold_maps_fail_a_float_comparison(shape):
    dl, dr = mo_case("threshold", *shape)
    assert (dl > 0).all() and (dl < 500).all() and np.array_equal(dl * 8, np.rint(dl * 8))
    bad = float_compare_disagrees(dl, dr)
    print(f"threshold {shape}: binary32 and binary64 comparisons disagree on {bad.mean():.3f} of the pixels")
    assert bad.mean() >= 0.05
    # ... and the disagreement is visible in the result: the map a float comparison would give is another map
    _, xr = column_of(dl)
    drs = np.take_along_axis(dr, xr, axis=1)
    z32 = (drs > f32(1.4) * dl) | (drs < f32(0.7) * dl)
    assert ((np.where(z32, f32(0), dl) != rule64(dl, dr)).mean()) >= 0.05


@pytest.mark.parametrize("shape", [(3, 255), (2, 256), (2, 257), (5, 513), (8, 47), (7, 257)])
def test_truncation_maps_fail_a_rounded_column(shape):
    dl, dr = mo_case("truncation", *shape)
    rows, cols = shape
    pos, xr = column_of(dl)
    fr = pos - np.floor(pos)
    for want in (0.5, 0.99, 0.0):
        assert (np.abs(fr - want) < 1e-3).mean() > 0.15, f"fraction {want} missing"
    assert (dl[:, 0] > 0).all() and (xr[:, 0] == 0).all()                      # dl > x: column 0
    assert (dl[:, cols - 2] == -1).all() and (pos[:, cols - 2] == cols - 1).all()  # a small negative: the last column, exactly
    other = rounding_selects_otherwise(dl, dr)
    print(f"truncation {shape}: rint and trunc select different dr on {other.mean():.3f} of the pixels")
    assert other.mean() >= 0.20
    # the selected value decides: with the rounded column the result is another map
    xn = np.clip(np.rint(pos).astype(np.int64), 0, cols - 1)
    drn = np.take_along_axis(dr, xn, axis=1).astype(np.float64)
    d = dl.astype(np.float64)
    with np.errstate(invalid="ignore"):
        zr = (drn > 1.4 * d) | (drn < 0.7 * d)
    assert (np.where(zr, f32(0), dl) != rule64(dl, dr)).mean() >= 0.15


def test_oracle_wrappers_refuse_out_of_row_maps(oracle, synth):
    for rows, cols in ((1, 1), (2, 257), (5, 513)):
        for what, m, _ in out_of_row_maps(rows, cols):
            with pytest.raises(ValueError):
                oracle.gpu_mask_occlusions(m, np.ones_like(m))
    # what the reference defines stays accepted
    ok = np.array([[np.nan, np.inf, -0.0, 1e-40, -3.0, 2.0, 1.0, 0.0]], np.float32)  # -3 at x = 4: column 7 of 8
    assert_bits(oracle.gpu_mask_occlusions(ok, np.ones_like(ok)), rule64(ok, np.ones_like(ok)), "accepted specials")
    p = synth.make_pair(3, rows=12, cols=20, n_points=6, dilate_factor=1)
    ims = oracle.ImageSet(p["left"], p["right"])
    for v in (-1.0, -1e-30, -np.inf):
        d = np.full((12, 20), 2.0, np.float32)
        d[5, 7] = v
        with pytest.raises(ValueError):
            oracle.gpu_mask_background(ims, d)
        with pytest.raises(ValueError):
            oracle.gpu_propagate(ims, d)
    d = np.full((12, 20), 2.0, np.float32)
    d[5, 7] = np.nan
    oracle.gpu_mask_background(ims, d)       # fmaxf(x - NaN, 1) = 1: in range
    with pytest.raises(ValueError):
        oracle.gpu_propagate(ims, d)         # !(d >= 0)


# ---- GPU helpers ----------------------------------------------------------------------------------------------------
def engine(pm, sem, rows, cols, batch=1, **kw):
    kw.setdefault("patch", 3)
    p = pm.default_params(sem, **kw)
    return pm.Engine(p, max_rows=max(rows, 8), max_cols=max(cols, 8), max_batch=batch)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def assert_refused(pm, e, call, buf, index):
    """The three checks of a refused map: PM_ERR_INVALID_ARG, the caller's buffer untouched, the index in pm_last_error."""
    before = buf.tobytes()
    assert call(buf) == pm.PM_ERR_INVALID_ARG
    assert buf.tobytes() == before, "a refused call wrote into the caller's map"
    msg = e.lib.pm_last_error(e.h).decode()
    assert f"[{index}]" in msg, msg
    return msg


# ---- GPU: pm_mask_occlusions ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", MO_SHAPES)
def test_mask_occlusions_map_families(pm, oracle, shape):
    rows, cols = shape
    with engine(pm, 1, rows, cols) as e:
        for family in FAMILIES:
            dl, dr = mo_case(family, rows, cols)
            assert_bits(e.mask_occlusions(dl, dr), oracle.gpu_mask_occlusions(dl, dr), f"{family} {shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1), (2, 257), (5, 513)])
def test_mask_occlusions_refuses_columns_past_the_row(pm, oracle, shape):
    rows, cols = shape
    good_l, good_r = mo_case("special", rows, cols)
    with engine(pm, 1, rows, cols) as e:
        for what, m, index in out_of_row_maps(rows, cols):
            dr = np.ones_like(m)
            msg = assert_refused(pm, e, lambda b: e.lib.pm_mask_occlusions(e.h, ptr(b), ptr(dr), rows, cols), m, index)
            assert "pm_mask_occlusions" in msg, what
            assert_bits(e.mask_occlusions(good_l, good_r), oracle.gpu_mask_occlusions(good_l, good_r),
                        f"a good call after the refusal of {what}")


# ---- GPU: k_seed -> background -> k_finalize through Match() with patchmatch_iters == 0 ------------------------------
# run_match (pm_engine.hip::view_op) runs ONE stage at 0 iterations in both semantics: the background mask, uncached.
# Its factor is set so that it keeps what it can (win_by_factor tiny / cost_improve_factor huge): the maps that reach
# the cross-check are then the seeds, and the comparison is against oracle.match at the same parameters.
KEEP = {0: dict(win_by_factor=1e-6), 1: dict(cost_improve_factor=1e6)}
OKEEP = {0: 1e-6, 1: 1e6}


def seed_case(rows, cols, k):
    """Seeds for (left, right): threshold, truncation maps, then cells of NaN, negatives and -0.0 (all |v| <= cols)."""
    rng = np.random.default_rng(100 * rows + cols + k)
    if k % 2 == 0:
        sl, sr = threshold_maps(rows, cols, 31 * rows + cols + k, dmax=min(500, cols))
    else:
        sl, sr = truncation_maps(rows, cols, 31 * rows + cols + k)
    sl, sr = sl.copy(), sr.copy()
    sr[np.isnan(sr)] = f32(1.0)
    for m in (sl, sr):
        pick = rng.integers(0, 16, m.shape)
        m[pick == 0] = np.nan
        m[pick == 1] = -rng.uniform(0.0, cols, int((pick == 1).sum())).astype(np.float32)
        m[pick == 2] = -0.0
    return np.clip(sl, -cols, cols), np.clip(sr, -cols, cols)


def images(rows, cols, k):
    rng = np.random.default_rng(5000 + 10 * rows + cols + k)
    return rng.integers(0, 256, (rows, cols), dtype=np.uint8), rng.integers(0, 256, (rows, cols), dtype=np.uint8)


def omatch(oracle, sem, iters, l, r, sl, sr, lr=1, patch=3, **kw):
    p = oracle.default_params(sem, patch=patch, n_iters=iters, left_right_check=lr, nthreads=4, **kw)
    return oracle.match(p, l, r, sl, sr if lr else None)


def clamped(seed):
    with np.errstate(invalid="ignore"):
        c = np.where(seed > 0, seed, f32(0)).astype(np.float32)
    assert not np.array_equal(c.view(np.uint32), seed.view(np.uint32))
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("rows", [5, 6, 7, 8])   # every remainder of the state planes' four-row interleave
@pytest.mark.parametrize("cols", [47, 257])
def test_finalize_cross_check_on_raw_seeds(pm, oracle, sem, rows, cols):
    l, r = images(rows, cols, 0)
    with engine(pm, sem, rows, cols, patchmatch_iters=0, left_right_check=1, **KEEP[sem]) as e:
        for k in (0, 1):
            sl, sr = seed_case(rows, cols, k)
            dl, dr = e.match(l, r, sl, sr)
            el, er = omatch(oracle, sem, 0, l, r, sl, sr, bg_factor=OKEEP[sem])
            assert_bits(dl, el, f"seeds {k}: left")
            assert_bits(dr, er, f"seeds {k}: right")
            # the case is what it claims: the seeds reach the cross-check (the right map IS the clamped seed wherever
            # the background stage kept it) and the cross-check decides on them
            kept = er != 0
            assert kept.mean() > 0.5 and np.array_equal(er[kept], np.maximum(sr, 0)[kept])
            assert (el != 0).mean() > 0.1 and ((el == 0) & (sl > 0)).mean() > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("sem", [0, 1])
def test_finalize_batch_of_three_and_strided_outputs(pm, oracle, sem):
    rows, cols = 7, 47
    pairs = [images(rows, cols, k) + seed_case(rows, cols, k) for k in range(3)]
    want = [omatch(oracle, sem, 0, *p, bg_factor=OKEEP[sem]) for p in pairs]
    with engine(pm, sem, rows, cols, batch=3, patchmatch_iters=0, left_right_check=1, **KEEP[sem]) as e:
        dls, drs = e.match_batch(*[[p[j] for p in pairs] for j in range(4)])   # pm_match_batch_u8: per-pair plane offsets
        for i in range(3):
            assert_bits(dls[i], want[i][0], f"batch slot {i} left")
            assert_bits(drs[i], want[i][1], f"batch slot {i} right")
        # pm_match_u8 with a disp_step wider than a row: the columns behind a row stay as they were
        step = cols + 5
        out_l = np.full((rows, step), -7.0, np.float32)
        out_r = np.full((rows, step), -7.0, np.float32)
        l, r, sl, sr = pairs[1]
        rc = e.lib.pm_match_u8(e.h, ptr(l), ptr(r), rows, cols, 0, ptr(sl), ptr(sr), 0, ptr(out_l), ptr(out_r), 4 * step)
        assert rc == pm.PM_OK, e.lib.pm_last_error(e.h).decode()
        assert_bits(out_l[:, :cols], want[1][0], "strided left")
        assert_bits(out_r[:, :cols], want[1][1], "strided right")
        assert (out_l[:, cols:] == -7.0).all() and (out_r[:, cols:] == -7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("sem", [0, 1])
def test_raw_seeds_equal_clamped_seeds_with_iterations(pm, oracle, sem):
    """Loading a seed as `s > 0 ? s : 0` changes nothing once a noise step runs: raw seeds (NaN, negatives, -0.0) and
    seeds clamped on the host give identical maps at patchmatch_iters = 2, and both equal the oracle."""
    rows, cols = 8, 47
    l, r = images(rows, cols, 9)
    sl, sr = seed_case(rows, cols, 1)
    cl, cr = clamped(sl), clamped(sr)
    with engine(pm, sem, rows, cols, patchmatch_iters=2, left_right_check=1) as e:
        raw = e.match(l, r, sl, sr)
        raw = (raw[0].copy(), raw[1].copy())
        pre = e.match(l, r, cl, cr)
    want = omatch(oracle, sem, 2, l, r, sl, sr)
    for got, what in ((raw, "raw seeds"), (pre, "clamped seeds")):
        assert_bits(got[0], want[0], f"{what}: left")
        assert_bits(got[1], want[1], f"{what}: right")


@pytest.mark.gpu
@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("rows", [5, 8])
def test_single_view_seed_kernel_on_raw_seeds(pm, oracle, sem, rows):
    """left_right_check = 0: the seeds go through k_seed (with two views the copy rides in k_prep).  At 0 iterations its
    `s > 0 ? s : 0` is all that stands between a negative seed and the background mask's sample position; at 2
    iterations raw and clamped seeds give the same map."""
    cols = 47
    l, r = images(rows, cols, 3)
    for k in (0, 1):
        sl, _ = seed_case(rows, cols, k)
        with engine(pm, sem, rows, cols, patchmatch_iters=0, left_right_check=0, **KEEP[sem]) as e:
            dl, _ = e.match(l, r, sl, None)
        el, _ = omatch(oracle, sem, 0, l, r, sl, None, lr=0, bg_factor=OKEEP[sem])
        assert_bits(dl, el, f"seeds {k}, 0 iterations")
        kept = el != 0
        assert kept.mean() > 0.5 and np.array_equal(el[kept], sl[kept])   # the map that comes back IS the clamped seed
        with engine(pm, sem, rows, cols, patchmatch_iters=2, left_right_check=0) as e:
            raw = e.match(l, r, sl, None)[0].copy()
            pre = e.match(l, r, clamped(sl), None)[0]
        want, _ = omatch(oracle, sem, 2, l, r, sl, None, lr=0)
        assert_bits(raw, want, f"seeds {k}, 2 iterations, raw")
        assert_bits(pre, want, f"seeds {k}, 2 iterations, clamped")


@pytest.mark.gpu
@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("eng", [1, 2, 5])      # PM_ENGINE_SERIAL, _WAVE, _RUNBLK2
@pytest.mark.parametrize("rows", [5, 6, 7])
def test_match_below_eight_rows_with_iterations(pm, oracle, sem, eng, rows):
    """Match() takes 5 rows and more: noise + cost, the four sweeps (chains of 3 and of 1 positions), the line planes of
    the run engine, the background mask and the cross-check at those heights against the oracle."""
    cols = 47
    l, r = images(rows, cols, 5)
    sl, sr = seed_case(rows, cols, 0)
    for patch in ((3, 5) if sem == 0 else (3,)):
        with engine(pm, sem, rows, cols, patch=patch, patchmatch_iters=2, left_right_check=1, engine=eng) as e:
            dl, dr = e.match(l, r, sl, sr)
        el, er = omatch(oracle, sem, 2, l, r, sl, sr, patch=patch)
        assert_bits(dl, el, f"{patch}x{patch}: left")
        assert_bits(dr, er, f"{patch}x{patch}: right")


# ---- GPU: pm_remove_background --------------------------------------------------------------------------------------
BG_WINDOWS = [(3, 3), (5, 5), (7, 7), (9, 9), (11, 11), (7, 3), (3, 9), (15, 15)]   # (pw, ph): every tiled kernel + generic
BG_SIZES = [(16, 64), (50, 90), (9, 33), (13, 24)]  # exact tiles; ragged; a short one; narrower than a 32-wide tile, 11x11 fits
FACTORS = tuple(float(2.0 ** (k / 4.0)) for k in range(-8, 17))   # 0.25 .. 16


@functools.lru_cache(maxsize=None)
def bg_pair(synth, rows, cols):
    p = synth.make_pair(200 + rows + cols, rows=rows, cols=cols, n_points=10, dilate_factor=1)
    return p["left"], p["right"], p["gt"]


def bg_dense_map(synth, rows, cols, special, amp=1.5):
    """Fractional disparities within `amp` of the pair's truth; a band of rows above x - pw/2, where the clamp applies;
    with `special`: cells of NaN, negatives and +inf (PM_SEM_CPU clamps them; the oracle defines the result)."""
    _, _, gt = bg_pair(synth, rows, cols)
    rng = np.random.default_rng(17 * rows + cols)
    d = (gt + rng.uniform(-amp, amp, gt.shape)).astype(np.float32)
    d = np.maximum(d, f32(0.125))
    band = slice(rows // 3, rows // 3 + max(2, rows // 5))
    xs = np.arange(cols, dtype=np.float32)[None, :]
    d[band] = (xs + rng.uniform(-3.0, 4.0, d[band].shape)).astype(np.float32).clip(0.125, None)
    if special:
        pick = rng.integers(0, 40, d.shape)
        d[pick == 0] = np.nan
        d[pick == 1] = -rng.uniform(0.0, 30.0, int((pick == 1).sum())).astype(np.float32)
        d[pick == 2] = np.inf
    return d


def interior_mask(rows, cols, pw, ph):
    m = np.zeros((rows, cols), bool)
    m[ph // 2:rows - ph // 2, pw // 2:cols - pw // 2] = True
    return m


def has_interior(size, window):
    return size[0] >= window[1] and size[1] >= window[0]


@functools.lru_cache(maxsize=None)
def bg_cpu_case(O, synth, rows, cols, pw, ph):
    """(dense map, factor, expected, kept share, interior pixels) with the factor chosen on the oracle O: the one of
    FACTORS whose kept share of the interior is nearest one half.  A window that does not fit the image has no interior:
    any factor leaves the map as it is."""
    l, r, _ = bg_pair(synth, rows, cols)
    ims = O.ImageSet(l, r)
    d = bg_dense_map(synth, rows, cols, special=False)
    inside = interior_mask(rows, cols, pw, ph)
    best = None
    for f in FACTORS:
        out = O.cpu_remove_background(ims, d, ph, pw, f)
        kept = float((out[inside] != 0).mean()) if inside.any() else 0.5
        if best is None or abs(kept - 0.5) < abs(best[0] - 0.5):
            best = (kept, f, out)
    return d, best[1], best[2], best[0], int(inside.sum())


@functools.lru_cache(maxsize=None)
def bg_gpu_case(O, synth, rows, cols):
    """The dense map of the PM_SEM_GPU cases: the widest jitter around the truth at which MaskBackground keeps between a
    quarter and three quarters of the interior at BOTH prescribed factors, 0.8 and 0.5 (chosen on the oracle O)."""
    l, r, _ = bg_pair(synth, rows, cols)
    ims = O.ImageSet(l, r)
    inside = interior_mask(rows, cols, 3, 3)
    for amp in (1.5, 1.25, 1.0, 0.75, 0.5, 0.375, 0.25, 0.125):
        d = bg_dense_map(synth, rows, cols, special=False, amp=amp)
        kept = [float((O.gpu_mask_background(ims, d, 0.9, f)[inside] != 0).mean()) for f in (0.8, 0.5)]
        if all(0.25 <= k <= 0.75 for k in kept):
            break
    return d, kept


DENSE_CASES = [(s, w) for w in BG_WINDOWS for s in BG_SIZES if has_interior(s, w)]
NO_INTERIOR = [(s, w) for w in BG_WINDOWS for s in BG_SIZES if not has_interior(s, w)]


@pytest.mark.parametrize("size,window", NO_INTERIOR)
def test_remove_background_leaves_a_map_without_interior(oracle, synth, size, window):
    d, _, out, _, n = bg_cpu_case(oracle, synth, *size, *window)
    assert n == 0 and np.array_equal(out, d)


@pytest.mark.parametrize("size", BG_SIZES)
def test_mask_background_dense_maps_keep_and_zero_a_quarter(oracle, synth, size):
    _, kept = bg_gpu_case(oracle, synth, *size)
    print(f"{size}: MaskBackground keeps {kept[0]:.3f} at factor 0.8, {kept[1]:.3f} at factor 0.5")
    assert all(0.25 <= k <= 0.75 for k in kept)


@pytest.mark.parametrize("size,window", DENSE_CASES)
def test_remove_background_factor_makes_the_threshold_matter(oracle, synth, size, window):
    rows, cols = size
    pw, ph = window
    d, factor, out, kept, n = bg_cpu_case(oracle, synth, rows, cols, pw, ph)
    assert n > 0
    print(f"{size} {pw}x{ph}: factor {factor:.3f} keeps {kept:.3f} of {n} interior pixels")
    assert (d[interior_mask(rows, cols, pw, ph)] != 0).all()   # dense
    assert kept >= 0.25 and 1.0 - kept >= 0.25


@pytest.mark.gpu
@pytest.mark.parametrize("size", BG_SIZES)
def test_remove_background_cpu_semantics_every_window(pm, oracle, synth, size):
    rows, cols = size
    l, r, _ = bg_pair(synth, rows, cols)
    ims = oracle.ImageSet(l, r)
    sp = bg_dense_map(synth, rows, cols, special=True)
    with engine(pm, 0, rows, cols) as e:
        for pw, ph in BG_WINDOWS:
            # (a window that does not fit the image -- NO_INTERIOR -- must leave every map untouched, whatever the factor)
            d, factor, want, _, _ = bg_cpu_case(oracle, synth, rows, cols, pw, ph)
            assert_bits(e.remove_background(l, r, d, ph, pw, factor), want, f"{size} {pw}x{ph} dense, factor {factor:.3f}")
            # factor 1: the pixels whose two costs are EQUAL (both capped at tau, or d clamped to 0) sit on the threshold
            for f in (1.0, factor):
                assert_bits(e.remove_background(l, r, sp, ph, pw, f), oracle.cpu_remove_background(ims, sp, ph, pw, f),
                            f"{size} {pw}x{ph} with NaN / negative / +inf cells, factor {f:.3f}")
            assert_bits(e.remove_background(l, r, d, ph, pw, 1.0), oracle.cpu_remove_background(ims, d, ph, pw, 1.0),
                        f"{size} {pw}x{ph} dense, factor 1")


@pytest.mark.gpu
@pytest.mark.parametrize("size", BG_SIZES)
def test_remove_background_gpu_semantics(pm, oracle, synth, size):
    rows, cols = size
    l, r, _ = bg_pair(synth, rows, cols)
    ims = oracle.ImageSet(l, r)
    d, _ = bg_gpu_case(oracle, synth, rows, cols)
    nan = d.copy()
    nan[::3, 1::4] = np.nan            # fmaxf(x - NaN, 1) = 1: accepted, and the oracle defines the result
    nan[1::5, 2::7] = np.inf
    with engine(pm, 1, rows, cols) as e:
        for f in (0.8, 0.5):
            want = oracle.gpu_mask_background(ims, d, 0.9, f)
            inside = interior_mask(rows, cols, 3, 3)
            assert 0.25 <= (want[inside] != 0).mean() <= 0.75   # the threshold keeps and zeroes a quarter at least
            assert_bits(e.remove_background(l, r, d, 3, 3, f), want, f"{size} dense, factor {f}")
            assert_bits(e.remove_background(l, r, nan, 3, 3, f), oracle.gpu_mask_background(ims, nan, 0.9, f),
                        f"{size} with NaN / +inf cells, factor {f}")
        for v, y, x in ((-1.0, rows - 2, cols - 2), (-np.inf, 1, 1), (-1e-30, rows // 2, cols // 2)):
            bad = d.copy()
            bad[y, x] = v
            call = lambda b: e.lib.pm_remove_background(e.h, ptr(l), ptr(r), rows, cols, ptr(b), 3, 3, 0.8)
            assert "pm_remove_background" in assert_refused(pm, e, call, bad, y * cols + x)
            assert_bits(e.remove_background(l, r, d, 3, 3, 0.8), oracle.gpu_mask_background(ims, d, 0.9, 0.8),
                        f"a good call after the refusal of {v}")


# ---- GPU: pm_propagate refusals, pm_add_noise on special values ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sem", [0, 1])
def test_propagate_refuses_values_below_zero_and_nan(pm, oracle, synth, sem):
    rows, cols = 16, 64
    l, r, gt = bg_pair(synth, rows, cols)
    ims = oracle.ImageSet(l, r)
    good = np.maximum(gt + f32(0.25), 0).astype(np.float32)
    want = oracle.cpu_propagate(ims, good, 3, 3, nthreads=4) if sem == 0 else oracle.gpu_propagate(ims, good, nthreads=4)
    with engine(pm, sem, rows, cols) as e:
        for v, y, x in ((-1.0, rows - 2, cols - 2), (np.nan, 3, 5), (-np.inf, 0, 0), (-1e-30, rows - 1, cols - 1)):
            bad = good.copy()
            bad[y, x] = v
            call = lambda b: e.lib.pm_propagate(e.h, ptr(l), ptr(r), rows, cols, ptr(b), 3, 3, 15)
            assert "pm_propagate" in assert_refused(pm, e, call, bad, y * cols + x)
            assert_bits(e.propagate(l, r, good, 3, 3, 15), want, f"semantics {sem}: a good call after the refusal of {v}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(8, 8), (9, 257)])
def test_add_noise_special_values(pm, oracle, shape):
    rows, cols = shape
    rng = np.random.default_rng(rows + cols)
    d = rng.uniform(0.0, 40.0, shape).astype(np.float32)
    vals = np.array([-1.0, -0.0, 0.0, np.nan, np.inf, -np.inf, 1e-40, -1e-40, 1e-30, 3e38, -3e38], np.float32)
    pick = rng.integers(0, 2 * len(vals), shape)
    d = np.where(pick < len(vals), vals[np.minimum(pick, len(vals) - 1)], d).astype(np.float32)
    with engine(pm, 1, rows, cols) as e:
        unit = e.unit_noise(rows, cols)
        for amp in (32.0, 0.5, 0.0):
            got = e.add_noise(d, amp)
            assert_bits(got, oracle.gpu_add_foreground_noise(d, unit, amp), f"AddForegroundNoise {amp}")
            with np.errstate(invalid="ignore"):
                mask = (d > 0).astype(np.uint8)
            assert_bits(got, oracle.cpu_add_noise(d, amp, mask), f"AddNoise {amp}")
