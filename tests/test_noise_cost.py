"""The noise + clamp + cost stage on its own, with its cost plane: k_noise_cost and k_noise_cost_tiled<W, W> through
pm_debug_noise_cost, and the background mask on a supplied cost plane (cached = 1) through pm_debug_remove_background
(include/pm/testing.h), against tests/noise_cost_ref.py pixel by pixel.

Every comparison is of bit patterns: the costs are exact by construction (integer SADs, mean_from_sum), so there is no
tolerance, and a sentinel in the cost plane shows which pixels the stage wrote.  Each tiled case asserts through
noise_cost_ref.tile_classes which branches of the tiled kernel its fields reach -- empty tiles, the four (ref_fast, tgt_fast)
fills, the whole-block fallback beyond the target span -- and a failure names the pixel, its tile and the tile's branch.

Which (ref_fast, tgt_fast) pairs a window can reach is geometry: a tile at x0 fills its reference tile fast iff
x0 - pw/2 - OFF >= 0 and x0 - pw/2 - OFF + 2 NPAIR <= cols, and the target span of its pixels ends at most at column
x0 + 32 + pw/2 (d = 0 in the tile's last column), so (True, False) needs x0 + 34 <= cols <= x0 + 35 for 3x3 and 5x5,
x0 + 36 <= cols <= x0 + 39 for 9x9, x0 + 38 <= cols <= x0 + 39 for 11x11 and is impossible for 7x7 (x0 + 36 <= cols < x0 + 36).
Of the prescribed shapes only 21 x 131 has such a tile (x0 = 96: 3x3 and 5x5); 12 x 70 is added for 9x9 and 11x11.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import noise_cost_ref as R

f32 = np.float32
SHAPES = [(8, 8), (9, 33), (13, 97), (21, 131), (19, 300)]
EXTRA_SHAPE = (12, 70)           # (True, False) for 9x9 and 11x11, see above
TILED = [(w, w) for w in R.TILED_WINDOWS]
GENERAL = [(13, 13), (15, 15), (7, 3), (3, 9)]      # (pw, ph): the general kernel
CONSTS = (32, 8, 224)            # what the shapes and fields here were laid out for
SENT = f32(-7.25)                # no cost is negative: an entry that still holds it was not written
FRACTIONS = [0.0, 2.0 ** -17, 0.25, 0.5, 1.0 - 2.0 ** -17, 1.0, 7.75]


def all_branches(pw):
    want = {"empty", "fallback", (False, False), (False, True), (True, True)}
    return want | ({(True, False)} if pw != 7 else set())


# ---- images and fields -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair(kind, rows, cols):
    if kind == "synth":
        import synth
        p = synth.make_pair(300 + rows + cols, rows=rows, cols=cols, n_points=10, dilate_factor=1)
        l, r = p["left"], p["right"]
    else:
        # "random": every byte value, so nearly every cost sits at its caps (tau_color, tau_grad) and the gradients beyond
        # 255 saturate; "narrow": twelve grey levels, so that neither mean reaches its cap and every tap counts
        rng = np.random.default_rng(9000 + 10 * rows + cols + (1 if kind == "narrow" else 0))
        lo, hi = (0, 256) if kind == "random" else (122, 134)
        l, r = rng.integers(lo, hi, (rows, cols), dtype=np.uint8), rng.integers(lo, hi, (rows, cols), dtype=np.uint8)
    l, r = np.ascontiguousarray(l), np.ascontiguousarray(r)
    l.setflags(write=False)
    r.setflags(write=False)
    return l, r


def kinds_for(shape):
    return ("random", "narrow", "synth") if shape[1] >= 97 else ("random", "narrow")


def columns(rows, cols):
    return np.arange(cols, dtype=np.float32)[None, :].repeat(rows, 0)


def mixed_field(rows, cols, pw, seed):
    """Per pixel one of: 0, a small value, a value within 2 of the clamp x - pw/2, one beyond it, anything in [0, x].  The
    last column of every tile and the last interior column hold 0: the largest first target column a tile can have."""
    rng = np.random.default_rng(seed)
    xs = columns(rows, cols)
    pick = rng.integers(0, 5, (rows, cols))
    d = np.zeros((rows, cols), np.float32)
    d = np.where(pick == 1, rng.uniform(0.0, 8.0, d.shape), d)
    d = np.where(pick == 2, xs - f32(pw // 2) - rng.uniform(0.0, 2.0, d.shape), d)
    d = np.where(pick == 3, xs + rng.uniform(0.0, 5.0, d.shape), d)
    d = np.where(pick == 4, xs * rng.random(d.shape), d)
    d = np.maximum(d, 0.0).astype(np.float32)
    d[:, CONSTS[0] - 1::CONSTS[0]] = 0
    if cols - pw // 2 - 1 >= 0:
        d[:, cols - pw // 2 - 1] = 0
    return np.ascontiguousarray(d)


def fraction_field(rows, cols, rot):
    """Constant per tile: tile k holds FRACTIONS[(k + rot) % 7]."""
    tw, th, _ = CONSTS
    ty, tx = np.arange(rows)[:, None] // th, np.arange(cols)[None, :] // tw
    k = (ty * ((cols + tw - 1) // tw) + tx + rot) % len(FRACTIONS)
    return np.asarray(FRACTIONS, np.float32)[k]


def span_field(rows, cols, pw):
    """19 x 300: the tile at x0 = 224 needs exactly target_span columns, its neighbour at x0 = 256 one more.  Two pixels of
    every row decide a tile's lo and hi (lo is not a multiple of four), the others lie between; all other tiles hold 0."""
    tw, _, span = CONSTS
    half = (pw - 1) // 2
    d = np.zeros((rows, cols), np.float32)
    xs = columns(rows, cols)
    for x0, lo4, extra in ((224, 32, 0), (256, 64, 1)):
        d[:, x0:x0 + tw] = xs[:, x0:x0 + tw] - f32(100 + half)             # ipx = 100
        d[:, x0] = x0 - (lo4 + 1) - half                                      # ipx = lo4 + 1
        hi = span + extra - 1 + lo4 - pw                                      # rw = hi + pw + 1 - lo4
        d[:, x0 + tw - 1] = (x0 + tw - 1) - hi - half
    assert (d >= 0).all() and (d <= xs - f32(pw // 2))[:, 224:288].all()
    return d


def special_field(rows, cols, pw, seed, negatives, nan):
    """mixed_field with cells beyond the clamp, 1e30, +inf, a denormal and -0.0; negatives: also -x values and -inf;
    nan: also NaN."""
    rng = np.random.default_rng(seed)
    d = mixed_field(rows, cols, pw, seed + 1)
    xs = columns(rows, cols)
    beyond = np.maximum(xs - f32(pw // 2) + rng.uniform(0.01, 5.0, d.shape).astype(np.float32), f32(0.01))
    vals = [beyond, f32(1e30), f32(np.inf), f32(1e-40), f32(-0.0)]
    if negatives:
        vals += [-rng.uniform(0.0, 40.0, d.shape).astype(np.float32), f32(-np.inf), f32(-1e-40)]
    if nan:
        vals += [f32(np.nan)]
    pick = rng.integers(0, 2 * len(vals), d.shape)
    for i, v in enumerate(vals):
        d = np.where(pick == i, v, d).astype(np.float32)
    return np.ascontiguousarray(d)


def clamped_for_predicate(d_in, pw, unit=None, amount=-1.0):
    return R.clamp_cpu(R.noise_step(d_in, unit, amount), pw)


def branches_of(d_in, pw, keep_zero=0, unit=None, amount=-1.0):
    rows, cols = d_in.shape
    return R.tile_classes(clamped_for_predicate(d_in, pw, unit, amount), pw, rows, cols, keep_zero, d_in=d_in, consts=CONSTS)


def every_window_fields(pw):
    """(shape, field) of test 1 for the tiled window pw."""
    return [(s, mixed_field(*s, pw, 7 * s[0] + s[1] + pw)) for s in SHAPES + [EXTRA_SHAPE]]


# ---- comparison --------------------------------------------------------------------------------------------------------
def assert_plane(got, want, what, tiles=None):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if len(bad):
        y, x = (int(v) for v in bad[0])
        where = ""
        if tiles is not None:
            tw, th, _ = CONSTS
            t = next(t for t in tiles if t.ty == y // th and t.tx == x // tw)
            where = f" in tile (ty={t.ty}, tx={t.tx}) of branch {R.branch(t)}, rw = {t.rw}, lane ({x % tw}, {y % th})"
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ; first at (y={y}, x={x}){where}: "
                             f"{got[y, x]!r} vs {want[y, x]!r}")


def run_case(e, O, sem, kind, d_in, pw, ph, amount=-1.0, keep_zero=0, cost_in=None, unit=None, what=""):
    """One call of the hook against the reference -> (disp, cost, tiles)."""
    rows, cols = d_in.shape
    l, r = pair(kind, rows, cols)
    ims = ims_of(O, kind, rows, cols)
    if cost_in is None:
        cost_in = np.full((rows, cols), SENT, np.float32)
    if amount >= 0 and unit is None:
        unit = e.unit_noise(rows, cols)
    got_d, got_c = e.debug_noise_cost(l, r, d_in, ph, pw, amount, keep_zero, cost_in)
    want_d, want_c = R.stage(O, ims, sem, d_in, pw, ph, amount, keep_zero, unit, cost_in)
    tiles = branches_of(d_in, pw, keep_zero, unit, amount) if R.is_tiled(sem, pw, ph) else None
    tag = f"{what} {kind} {rows}x{cols} window {pw}x{ph} semantics {sem} amount {amount} keep_zero {keep_zero}"
    assert_plane(got_d, want_d, tag + ": disp", tiles)
    assert_plane(got_c, want_c, tag + ": cost", tiles)
    return got_d, got_c, tiles


_IMS = {}


def ims_of(O, kind, rows, cols):
    key = (kind, rows, cols)
    if key not in _IMS:
        _IMS[key] = O.ImageSet(*pair(kind, rows, cols))
    return _IMS[key]


def engine(pm, sem, **kw):
    kw.setdefault("patch", 3)
    return pm.Engine(pm.default_params(sem, **kw), max_rows=24, max_cols=304, max_batch=1)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- CPU only: the constants, the predicate, the reference's own consistency, the coverage of the fields ---------------
def test_exported_constants_are_what_the_shapes_were_chosen_for(pm):
    assert "pm_debug_noise_cost_constants" in pm.EXPORTS and "pm_debug_noise_cost" in pm.EXPORTS
    assert "pm_debug_remove_background" in pm.EXPORTS
    assert pm.noise_cost_constants() == CONSTS, "tile geometry changed: re-derive SHAPES, span_field and the docstring"


def test_tile_classes_on_hand_worked_tiles():
    # 3x3 on 9 x 33, d = 0: interior x 1..31, y 1..7; ipx = x - 1
    t = R.tile_classes(np.zeros((9, 33), np.float32), 3, 9, 33, 0, consts=CONSTS)
    assert [(a.ty, a.tx) for a in t] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    # lo = 0, hi = 30, rw = 30 + 3 + 1 - 0; reference tile from column -2: slow; target columns 0 .. 35 > 33: slow
    assert t[0] == R.Tile(0, 0, "tiled", False, False, 34, 0, 30, frozenset({0, 1, 2, 3}))
    assert [a.kind for a in t[1:]] == ["empty"] * 3           # column 32 and row 8 lie outside the interior
    # 5x5 on 8 x 131, d = 0: interior x 2..128, y 2..5; ipx = x - 2
    t = R.tile_classes(np.zeros((8, 131), np.float32), 5, 8, 131, 0, consts=CONSTS)
    # x0 = 96: lo = 94, hi = 125, lo4 = 92, rw = 125 + 6 - 92; reference columns 94 .. 129 <= 131: fast; target 92 .. 131: slow
    assert t[3] == R.Tile(0, 3, "tiled", True, False, 39, 94, 125, frozenset({0, 1, 2, 3}))
    # x0 = 128: only x = 128: ipx = 126, lo4 = 124, rw = 8; reference columns 126 .. 161: slow; target 124 .. 131: slow
    assert t[4] == R.Tile(0, 4, "tiled", False, False, 8, 126, 126, frozenset({2}))
    assert R.branch(t[0]) == (False, True) and t[0].rw == 29 + 6   # x0 = 0: lo = 0, hi = 29
    # 3x3 on 8 x 300: one pixel at d = 0.5 (ipx = floor(256 - 0.5 - 1) = 254) and one at its clamp (ipx = 0) in the tile at
    # x0 = 256; with keep_zero they are the only pixels evaluated: rw = 254 + 4 - 0 > 224
    d = np.zeros((8, 300), np.float32)
    d[1, 256], d[1, 287] = 0.5, 286.0
    t = R.tile_classes(d, 3, 8, 300, 1, d_in=d, consts=CONSTS)
    assert t[8] == R.Tile(0, 8, "fallback", None, None, 258, 0, 254, frozenset({0, 2}))
    assert all(a.kind == "empty" for a in t[:8] + t[9:])
    t = R.tile_classes(d, 3, 8, 300, 0, consts=CONSTS)
    assert t[8].kind == "fallback" and t[8].rw == 286 + 4 and t[0].kind == "tiled"
    # a window that does not fit: nothing but empty tiles
    assert all(a.kind == "empty" for a in R.tile_classes(np.zeros((8, 8), np.float32), 9, 8, 8, 0, consts=CONSTS))
    # 2^-17 below 64 <= x < 128 is representable (ipx = x - 2), from 128 on x - 2^-17 rounds back to x (ipx = x - 1)
    ipx = R.first_target_column(np.full((1, 300), 2.0 ** -17, np.float32), 3)
    assert ipx[0, 100] == 98 and ipx[0, 200] == 199


@pytest.mark.parametrize("pw", R.TILED_WINDOWS)
def test_fields_reach_the_branches_they_claim(pw):
    seen = set()
    for shape, d in every_window_fields(pw):
        seen |= {R.branch(t) for t in branches_of(d, pw)}
    assert seen == all_branches(pw), (pw, seen)
    # the (True, False) fill on the prescribed shapes: 3x3 and 5x5 only
    on_prescribed = {R.branch(t) for s, d in every_window_fields(pw)[:-1] for t in branches_of(d, pw)}
    assert ((True, False) in on_prescribed) == (pw in (3, 5))
    # fractions: every byte shift of the target read within one tile, on both shapes
    for shape in ((13, 97), (19, 300)):
        for rot in range(len(FRACTIONS)):
            tiles = branches_of(fraction_field(*shape, rot), pw)
            assert any(t.kind == "tiled" and t.shifts == frozenset({0, 1, 2, 3}) for t in tiles)
    # the span edge
    by_x0 = {t.tx * CONSTS[0]: t for t in branches_of(span_field(19, 300, pw), pw) if t.ty == 0}
    assert by_x0[224].kind == "tiled" and by_x0[224].rw == CONSTS[2] and by_x0[224].lo % 4 == 1
    assert by_x0[256].kind == "fallback" and by_x0[256].rw == CONSTS[2] + 1


def test_reference_self_checks(oracle):
    rows, cols = 13, 97
    ims = ims_of(oracle, "narrow", rows, cols)
    rng = np.random.default_rng(5)
    # the two forms of the oracle's cost agree where the stage evaluates: clamped d, every fraction of FRACTIONS
    for pw, ph in ((3, 3), (7, 7), (11, 11), (7, 3), (15, 15)):
        d = R.clamp_cpu(mixed_field(rows, cols, pw, 3) + np.asarray(FRACTIONS, np.float32)[rng.integers(0, 7, (rows, cols))], pw)
        ys, xs = np.nonzero(R.interior_mask(0, rows, cols, pw, ph))
        for i in rng.choice(len(ys), min(150, len(ys)), replace=False):
            x, y = int(xs[i]), int(ys[i])
            a = oracle.cpu_cost(ims, pw, ph, x, y, float(d[y, x]), literal=False)
            b = oracle.cpu_cost(ims, pw, ph, x, y, float(d[y, x]), literal=True)
            assert f32(a).view(np.uint32) == f32(b).view(np.uint32), (pw, ph, x, y, d[y, x], a, b)
    # the noise rule is AddForegroundNoise
    d = special_field(rows, cols, 3, 11, negatives=True, nan=True)
    unit = rng.uniform(-1, 1, d.shape).astype(np.float32)
    unit[0, :4] = (-1.0, 0.0, -0.0, 1.0)
    for amount in (0.0, 0.125, 1.0, 8.0):
        assert_plane(R.noise_step(d, unit, amount), oracle.gpu_add_foreground_noise(d, unit, amount), f"noise {amount}")
    assert_plane(R.noise_step(d, unit, -1.0), d, "no noise")
    # the background rule without a plane is the oracle's; with the plane of the true costs it is again
    d = special_field(rows, cols, 5, 13, negatives=True, nan=True)
    want = oracle.cpu_remove_background(ims, d, 5, 5, 1.5)
    assert_plane(R.background(oracle, ims, 0, d, None, 5, 5, 1.5), want, "RemoveBackground restated")
    _, true_cost = R.stage(oracle, ims, 0, d, 5, 5, -1.0, 0, None, np.full(d.shape, SENT))
    assert_plane(R.background(oracle, ims, 0, d, true_cost, 5, 5, 1.5), want, "RemoveBackground on the true costs")
    dg = special_field(rows, cols, 3, 17, negatives=False, nan=True)
    want = oracle.gpu_mask_background(ims, dg, 0.9, 0.8)
    assert_plane(R.background(oracle, ims, 1, dg, None, 3, 3, 0.8), want, "MaskBackground restated")
    _, true_cost = R.stage(oracle, ims, 1, dg, 3, 3, -1.0, 0, None, np.full(dg.shape, SENT))
    assert_plane(R.background(oracle, ims, 1, dg, true_cost, 3, 3, 0.8), want, "MaskBackground on the true costs")


# ---- 1. every window, no noise ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("window", TILED + GENERAL)
def test_every_window_no_noise_cpu_semantics(pm, oracle, window):
    pw, ph = window
    seen = set()
    with engine(pm, 0) as e:
        for shape, d in every_window_fields(pw):
            for kind in kinds_for(shape):
                _, cost, tiles = run_case(e, oracle, 0, kind, d, pw, ph)
                inside = R.interior_mask(0, *shape, pw, ph)
                assert (cost[~inside] == SENT).all() and (cost[inside] >= 0).all()
                if tiles:
                    seen |= {R.branch(t) for t in tiles}
    if window in TILED:
        assert seen == all_branches(pw), seen


@pytest.mark.gpu
def test_every_shape_no_noise_gpu_semantics(pm, oracle):
    with engine(pm, 1) as e:
        for shape in SHAPES:
            d = mixed_field(*shape, 3, 5 * shape[0] + shape[1])
            d[1::3, 2::5] = np.nan            # fmaxf(x - NaN, 1) = 1: accepted without noise
            for kind in kinds_for(shape):
                _, cost, _ = run_case(e, oracle, 1, kind, d, 3, 3)
                inside = R.interior_mask(1, *shape, 3, 3)
                assert (cost[~inside] == SENT).all() and (cost[inside] >= 0).all()


# ---- 2. fractions and byte shifts ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("window", TILED)
@pytest.mark.parametrize("shape", [(13, 97), (19, 300)])
def test_fractions_constant_per_tile(pm, oracle, window, shape):
    pw, ph = window
    with engine(pm, 0) as e:
        for rot in range(len(FRACTIONS)):
            _, _, tiles = run_case(e, oracle, 0, "narrow", fraction_field(*shape, rot), pw, ph, what=f"rotation {rot}")
            assert any(t.kind == "tiled" and t.shifts == frozenset({0, 1, 2, 3}) for t in tiles)


# ---- 3. the span edge --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("window", TILED)
def test_target_span_edge(pm, oracle, window):
    pw, ph = window
    with engine(pm, 0) as e:
        for kind in ("random", "narrow", "synth"):
            _, _, tiles = run_case(e, oracle, 0, kind, span_field(19, 300, pw), pw, ph)
            by_x0 = {t.tx * CONSTS[0]: t for t in tiles if t.ty == 0}
            assert by_x0[224].kind == "tiled" and by_x0[224].rw == CONSTS[2]
            assert by_x0[256].kind == "fallback" and by_x0[256].rw == CONSTS[2] + 1


# ---- 4. clamp and special values -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("window", TILED + [(15, 15)])
def test_special_values_cpu_semantics(pm, oracle, window):
    pw, ph = window
    with engine(pm, 0) as e:
        for shape in ((9, 33), (21, 131)):
            d = special_field(*shape, pw, 50 + pw, negatives=True, nan=True)
            for amount in (-1.0, 1.0):
                got, _, _ = run_case(e, oracle, 0, "narrow", d, pw, ph, amount=amount)
                outside = ~R.interior_mask(0, *shape, pw, ph)
                if amount < 0:   # returned bit for bit where the stage does not clamp
                    assert np.array_equal(got.view(np.uint32)[outside], d.view(np.uint32)[outside])
                    assert np.isnan(got[outside]).any() and (got[outside] < 0).any()


@pytest.mark.gpu
def test_special_values_gpu_semantics(pm, oracle):
    with engine(pm, 1) as e:
        for shape in ((9, 33), (21, 131)):
            run_case(e, oracle, 1, "narrow", special_field(*shape, 3, 60, negatives=False, nan=True), 3, 3, amount=-1.0)
            run_case(e, oracle, 1, "narrow", special_field(*shape, 3, 61, negatives=True, nan=True), 3, 3, amount=1.0)


# ---- 5. noise ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sem,window", [(0, (3, 3)), (0, (7, 7)), (0, (11, 11)), (0, (7, 3)), (1, (3, 3))])
def test_noise_amounts_with_the_handles_noise(pm, oracle, sem, window):
    pw, ph = window
    with engine(pm, sem) as e:
        for shape in ((13, 97), (19, 300)):
            d = mixed_field(*shape, pw, 70 + pw)
            d[::2, 1::3] = f32(1e-3)
            for amount in (0.0, 0.125, 1.0, 8.0):
                for kz in ((0, 1) if R.is_tiled(sem, pw, ph) else (0,)):
                    got, cost, _ = run_case(e, oracle, sem, "narrow", d, pw, ph, amount=amount, keep_zero=kz)
            # d = 1e-3 under amount 1: about half fall to 0 and are still evaluated, at 0 (the last call: amount 8 -> rerun at 1)
            got, cost, _ = run_case(e, oracle, sem, "narrow", d, pw, ph, amount=1.0, keep_zero=1 if sem == 0 and pw == ph else 0)
            small = (d == f32(1e-3)) & R.interior_mask(sem, *shape, pw, ph)
            fell = small & (got == 0)
            assert 0.25 < fell.sum() / small.sum() < 0.75 and (cost[fell] != SENT).all()


@pytest.mark.gpu
@pytest.mark.parametrize("sem,window", [(0, (5, 5)), (0, (9, 9)), (0, (13, 13)), (1, (3, 3))])
def test_injected_noise_sums_to_zero_and_below(pm, oracle, sem, window):
    pw, ph = window
    rows, cols = 21, 131
    rng = np.random.default_rng(80 + pw)
    unit = rng.choice(np.array([-1.0, -0.5, -0.25, 0.0, 0.5], np.float32), (rows, cols))
    d = rng.choice(np.array([0.5, 1.0, 2.0, 3.0], np.float32), (rows, cols))   # amount 2: s = d + 2 u in {-1.5 .. 4}
    s = d + 2 * unit
    assert (s == 0).mean() > 0.1 and (s < 0).mean() > 0.1 and (s > 0).mean() > 0.3
    with engine(pm, sem) as e:
        e.set_unit_noise(unit)
        assert_plane(e.unit_noise(rows, cols), unit, "injected unit noise")
        for kz in ((0, 1) if R.is_tiled(sem, pw, ph) else (0,)):
            got, cost, _ = run_case(e, oracle, sem, "narrow", d, pw, ph, amount=2.0, keep_zero=kz, unit=unit)
            inside = R.interior_mask(sem, rows, cols, pw, ph)
            assert (got[s <= 0] == 0).all() and not np.signbit(got).any()
            assert (cost[inside & (s <= 0)] != SENT).all()      # positive before the noise: evaluated at 0, keep_zero or not


# ---- 6. keep_zero ------------------------------------------------------------------------------------------------------------
def keep_zero_field(rows, cols, pw, seed):
    """Tile columns in turn: entirely "zero" (0, -0.0, NaN, negatives), "zero" but for ONE positive pixel, mixed."""
    tw, th, _ = CONSTS
    rng = np.random.default_rng(seed)
    zeros = rng.choice(np.array([0.0, -0.0, np.nan, -3.5, -np.inf], np.float32), (rows, cols))
    d = np.where(rng.random((rows, cols)) < 0.5, mixed_field(rows, cols, pw, seed + 1), zeros).astype(np.float32)
    for tx in range((cols + tw - 1) // tw):
        sl = slice(tx * tw, min(cols, (tx + 1) * tw))
        if tx % 3 != 2:
            d[:, sl] = zeros[:, sl]
        if tx % 3 == 1:
            for y in range(pw // 2, rows - pw // 2, th):     # one positive interior pixel per tile of this column
                d[y, min(sl.start + 5 + pw // 2, cols - pw // 2 - 1)] = f32(2.25)
    return np.ascontiguousarray(d)


@pytest.mark.gpu
@pytest.mark.parametrize("window", TILED)
@pytest.mark.parametrize("amount", [-1.0, 1.0])
def test_keep_zero(pm, oracle, window, amount):
    pw, ph = window
    with engine(pm, 0) as e:
        for shape in ((13, 97), (21, 131), (19, 300)):
            d = keep_zero_field(*shape, pw, 90 + pw)
            d0, c0, t0 = run_case(e, oracle, 0, "narrow", d, pw, ph, amount=amount, keep_zero=0)
            d1, c1, t1 = run_case(e, oracle, 0, "narrow", d, pw, ph, amount=amount, keep_zero=1)
            inside = R.interior_mask(0, *shape, pw, ph)
            zero_in = inside & ~R.positive(d)
            assert zero_in.any() and np.isnan(d[zero_in]).any() and np.signbit(d[zero_in]).any()
            assert (c1[zero_in] == SENT).all() and (c0[zero_in] != SENT).all()
            assert (d1[zero_in].view(np.uint32) == 0).all()                        # +0, whatever the input was
            assert_plane(d1, d0, "disp under keep_zero 1 vs 0")
            # tiles that return early beside tiles that evaluate a single pixel
            kinds0, kinds1 = [t.kind for t in t0], [t.kind for t in t1]
            assert kinds1.count("empty") > kinds0.count("empty")
            assert any(a == "tiled" and b == "empty" for a, b in zip(kinds0, kinds1))
            assert any(t.kind == "tiled" and t.lo == t.hi for t in t1)
            # the exactness claim: on a plane that holds the true costs of the zero pixels both give the same plane
            _, c2, _ = run_case(e, oracle, 0, "narrow", d, pw, ph, amount=amount, keep_zero=1, cost_in=c0)
            assert_plane(c2, c0, "cost under keep_zero 1 on the plane keep_zero 0 left")


@pytest.mark.gpu
def test_keep_zero_is_ignored_by_the_general_kernel(pm, oracle):
    d = keep_zero_field(13, 97, 7, 99)
    with engine(pm, 0) as e:
        a = run_case(e, oracle, 0, "narrow", d, 7, 3, amount=1.0, keep_zero=1)
        b = run_case(e, oracle, 0, "narrow", d, 7, 3, amount=1.0, keep_zero=0)
        assert_plane(a[1], b[1], "7x3 cost, keep_zero 1 vs 0")
    with engine(pm, 1) as e:
        run_case(e, oracle, 1, "narrow", d, 3, 3, amount=1.0, keep_zero=1)


# ---- 7. what Match() and pm_propagate run ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sem", [0, 1])
def test_hook_equals_propagate_without_a_pass(pm, oracle, sem):
    rows, cols = 21, 131
    l, r = pair("synth", rows, cols)
    d = mixed_field(rows, cols, 7, 123)
    with engine(pm, sem) as e:
        got, _ = e.debug_noise_cost(l, r, d, 7, 7, -1.0, 0, None)          # no cost plane in or out
        assert_plane(got, e.propagate(l, r, d, 7, 7, 0), "pm_debug_noise_cost vs pm_propagate(pass_mask = 0)")
        got2, _, _ = run_case(e, oracle, sem, "synth", d, 7, 7)
        assert_plane(got2, got, "with and without a cost plane")


# ---- 8. the background mask on a supplied cost plane ---------------------------------------------------------------------------
def decisive_plane(rows, cols, seed):
    """0 keeps whatever the images say (0 > thr never holds, 0 < thr unless thr is 0), 1e30 zeroes."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0.0, 1e30], np.float32), (rows, cols))


@pytest.mark.gpu
@pytest.mark.parametrize("window", TILED + [(15, 15), (7, 3)])
def test_background_with_a_cached_plane_cpu_semantics(pm, oracle, window):
    pw, ph = window
    with engine(pm, 0) as e:
        for shape in ((13, 97), (21, 131)):
            rows, cols = shape
            l, r = pair("narrow", rows, cols)
            ims = ims_of(oracle, "narrow", rows, cols)
            d = special_field(rows, cols, pw, 200 + pw, negatives=True, nan=True)
            d[1::2, ::3] = np.minimum(d[1::2, ::3], 6.0)                # many pixels inside the clamp: clamp(d) == d
            plane = decisive_plane(rows, cols, 300 + pw)
            for factor in (1.5, 1.0):
                want = R.background(oracle, ims, 0, d, plane, pw, ph, factor)
                assert_plane(e.debug_remove_background(l, r, d, plane, ph, pw, factor), want,
                             f"{shape} {pw}x{ph} cached, factor {factor}")
                plain = oracle.cpu_remove_background(ims, d, ph, pw, factor)
                assert_plane(e.debug_remove_background(l, r, d, None, ph, pw, factor), plain,
                             f"{shape} {pw}x{ph} null plane")
            # the plane decided: where clamp(d) == d (-0.0 included) the result follows it, elsewhere the images
            inside = R.interior_mask(0, rows, cols, pw, ph)
            if not inside.any():                       # 15x15 on 13 rows: the map comes back as it went in
                assert_plane(want, d, "no interior")
                continue
            used = inside & (R.clamp_cpu(d, pw) == d)
            assert 0.2 < used.sum() / inside.sum() < 0.9 and (used & np.signbit(d) & (d == 0)).any()
            kept = used & (plane == 0)
            assert (want[used & (plane > 0)] == 0).all() and np.array_equal(want[kept], d[kept])
            assert (want != plain)[used].mean() > 0.2          # ... and it is not what the images alone would give
            assert np.array_equal(want.view(np.uint32)[~used], plain.view(np.uint32)[~used])


@pytest.mark.gpu
def test_background_with_a_cached_plane_gpu_semantics(pm, oracle):
    with engine(pm, 1) as e:
        for shape in ((13, 97), (21, 131)):
            rows, cols = shape
            l, r = pair("narrow", rows, cols)
            ims = ims_of(oracle, "narrow", rows, cols)
            d = special_field(rows, cols, 3, 400, negatives=False, nan=True)
            plane = decisive_plane(rows, cols, 401)
            for factor in (0.8, 0.5):
                want = R.background(oracle, ims, 1, d, plane, 3, 3, factor)
                assert_plane(e.debug_remove_background(l, r, d, plane, 3, 3, factor), want,
                             f"{shape} cached, factor {factor}")
                plain = oracle.gpu_mask_background(ims, d, 0.9, factor)
                assert_plane(e.debug_remove_background(l, r, d, None, 3, 3, factor), plain, f"{shape} null plane")
            inside = R.interior_mask(1, rows, cols, 3, 3)
            assert (want[inside & (plane > 0)] == 0).all() and (want != plain)[inside].mean() > 0.2


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sem", [0, 1])
def test_refusals_leave_the_handle_usable(pm, oracle, sem):
    torch = pytest.importorskip("torch")
    rows, cols = 13, 97
    l, r = pair("random", rows, cols)
    d = mixed_field(rows, cols, 5, 500)
    cost = np.full((rows, cols), SENT, np.float32)
    with engine(pm, sem, patch=5 if sem == 0 else 3, patchmatch_iters=1) as e:
        def call(left=l, right=r, disp=d, plane=cost, ph=5, pw=5, amount=-1.0, kz=0):
            buf = disp.copy() if disp is not None else None
            opt = lambda a: ptr(a) if a is not None else None
            rc = e.lib.pm_debug_noise_cost(e.h, opt(left), opt(right), rows, cols, opt(buf), ptr(plane), ph, pw, amount, kz)
            if buf is not None:
                assert buf.tobytes() == disp.tobytes(), "a refused call wrote into the caller's map"
            return rc
        bad = [dict(left=None), dict(right=None), dict(disp=None), dict(amount=float("nan")), dict(kz=2), dict(kz=-1)]
        if sem == 0:
            bad += [dict(pw=4), dict(ph=1), dict(pw=17)]
        else:
            neg = d.copy()
            neg[rows - 2, cols - 2] = -1.0
            bad += [dict(disp=neg)]
        for kw in bad:
            assert call(**kw) == pm.PM_ERR_INVALID_ARG, kw
            assert b"pm_debug_noise_cost" in e.lib.pm_last_error(e.h) or "pw" in kw or "ph" in kw, kw
            assert (cost == SENT).all()
            run_case(e, oracle, sem, "random", d, 5, 5, what=f"after the refusal of {kw}")
        if sem == 1:   # with noise the same map is defined
            run_case(e, oracle, 1, "random", neg, 3, 3, amount=1.0)
        lib, bad_arg = e.lib, pm.PM_ERR_INVALID_ARG
        assert lib.pm_debug_noise_cost(None, ptr(l), ptr(r), rows, cols, ptr(d.copy()), None, 5, 5, -1.0, 0) == bad_arg
        assert lib.pm_debug_remove_background(e.h, ptr(l), ptr(r), rows, cols, None, ptr(cost), 5, 5, 1.5) == bad_arg
        # while capturing: a recorded Match() around the refused calls, as tests/test_gpu_parity.py captures it
        dev = torch.device("cuda:0")
        t = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)      # (a copy: the cached images are read-only)
        L, Rr, S = t(l), t(r), t(d)
        DL, DR = torch.empty_like(S), torch.empty_like(S)
        run = lambda: e.match_device(1, L.data_ptr(), Rr.data_ptr(), rows, cols, S.data_ptr(), S.data_ptr(), DL.data_ptr(),
                                     DR.data_ptr())
        run()
        e.synchronize()
        first = DL.cpu().numpy()
        e.capture_begin()
        assert call() == pm.PM_ERR_BUSY and b"pm_debug_noise_cost" in e.lib.pm_last_error(e.h)
        assert lib.pm_debug_remove_background(e.h, ptr(l), ptr(r), rows, cols, ptr(d.copy()), ptr(cost), 5, 5,
                                              1.5) == pm.PM_ERR_BUSY
        run()
        e.capture_end()
        e.replay()
        e.synchronize()
        assert_plane(DL.cpu().numpy(), first, "replay after the refused calls")
        run_case(e, oracle, sem, "random", d, 5, 5, what="after the capture")
