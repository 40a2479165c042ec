"""The device seeder stage by stage (csrc/pm_seed.hpp), and the host function that plans its launches.

tests/test_seed.py compares the END of the seeder -- the dilated seed map -- with the oracle.  Here every part is compared
on its own, bit for bit, through the hooks of include/pm/testing.h: the plan (pm_debug_seed_plan, no device), the response
plane, its maximum and the candidate keys (pm_debug_seed_trace), the selection on synthetic keys on every route the
parameters allow (pm_debug_seed_select), the matcher on corners at every border (pm_debug_seed_match) and the splat on
corners an image would not produce (pm_debug_seed_splat).  The definitions are the oracle's functions and, between them,
tests/seed_ref.py, which the CPU tests at the top pin to the oracle's composed detector and seed maps.
"""

import numpy as np
import pytest

import seed_ref
from conftest import assert_same

FUSED, GRID, LIST = 1, 2, 3          # pm_debug_seed_plan_record.route
ROUTES = (FUSED, GRID, LIST)
LDS_LIMIT = 150 * 1024


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what):
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ; first at {bad[0].tolist()}: " \
                          f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def noise_image(seed, rows, cols):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


def periodic_image(seed, rows, cols, py=5, px=7):
    tile = np.random.default_rng(seed).integers(0, 256, (py, px), dtype=np.uint8)
    return np.tile(tile, (rows // py + 1, cols // px + 1))[:rows, :cols].copy()


# ---- the restatement of tests/seed_ref.py against the oracle's composed functions (CPU) ------------------------------------
def _images(synth):
    return {"scene": synth.make_pair(3, rows=120, cols=200)["left"], "noise": noise_image(1, 96, 160),
            "periodic": periodic_image(35, 60, 70)}


@pytest.mark.parametrize("kind", ["scene", "noise", "periodic"])
@pytest.mark.parametrize("harris", [0, 1])
def test_candidates_and_greedy_selection_compose_to_the_oracles_detector(oracle, synth, kind, harris):
    img = _images(synth)[kind]
    for kw in (dict(), dict(min_distance=3, max_features=1024, quality_level=0.001), dict(min_distance=0, max_features=50),
               dict(block_size=9, min_distance=7, max_features=17)):
        sp = oracle.seed_params(use_harris=harris, **kw)
        resp = oracle.corner_response_map(img, sp.block_size, harris, sp.harris_k)
        got = seed_ref.greedy_select(seed_ref.candidates(resp, sp.quality_level), sp.min_distance, sp.max_features)
        xs, ys = oracle.gftt_detect(img, sp)
        assert got == list(zip(xs.tolist(), ys.tolist())), (kind, harris, kw)
        assert len(got) > 0


def _matches(oracle, left, right, sp):
    xs, ys = oracle.gftt_detect(left, sp)
    d = [oracle.match_rectified(left, right, float(x), float(y), sp) for x, y in zip(xs, ys)]
    return np.stack([xs, ys], axis=1), np.array(d, np.float32)


def test_splat_composes_to_the_oracles_seed_maps(oracle, synth):
    p = synth.make_pair(8, rows=119, cols=197)
    l, r = p["left"], p["right"]
    sp = oracle.seed_params()
    xy, d = _matches(oracle, l, r, sp)
    assert (d > 0).any() and (d < 0).any()
    for f in (0, 2, 4):
        assert_same(seed_ref.splat(xy, d, 119, 197, 2 ** f + 1), oracle.sparse_init(l, r, f, sp), f"SparseInit f={f}")
    for f in (1, 2, 3):
        got = seed_ref.splat(xy, d, 119, 197, 2 ** (f - 1) + 1, 2.0 ** -f, out_shape=(119 // f, 197 // f))
        assert_same(got, oracle.cpu_initialize(l, r, f, sp), f"Initialize f={f}")


# ---- the plan (CPU) --------------------------------------------------------------------------------------------------------
def fused_lds(gx, gy):
    return 8 * 2 * 2048 + 4 * (2048 + 64 + 8) + 16 * (gx + 2) * (gy + 2)


def plan(pm, rows, cols, forced=0, **kw):
    names = dict(md="min_distance_btw_features", maxf="max_features_per_frame", block="gftt_block_size")
    return pm.seed_plan(pm.default_params(1, **{names.get(k, k): v for k, v in kw.items()}), rows, cols, forced)


def refused(pm, rows, cols, forced, **kw):
    with pytest.raises(pm.PmError) as e:
        plan(pm, rows, cols, forced, **kw)
    return e.value.status == pm.PM_ERR_INVALID_ARG


@pytest.mark.parametrize("rows, cols, md, route, gx, gy, lds", [
    (720, 1280, 20, FUSED, 64, 36, fused_lds(64, 36)),   # the default: 81 376 bytes
    (720, 1280, 10, GRID, 128, 72, 128 * 72 * 16),       # tests/test_seed.py::test_sorted_fallback_selection: 147 456
    (720, 1280, 8, LIST, 160, 90, 0),                    # ... and its list case: the grid alone would take 230 400
    (720, 1280, 0, LIST, 0, 0, 0), (720, 1280, -3, LIST, 0, 0, 0),   # no min distance: the list accepts everything
    (480, 752, 1, LIST, 752, 480, 0),                    # test_selection_across_many_chunks (1024, 1): a grid of 5.7 MB
    (480, 752, 40, FUSED, 19, 12, fused_lds(19, 12)),   # ... (300, 40)
    (150, 260, 3, FUSED, 87, 50, fused_lds(87, 50)),     # the largest case of the selection tests below
    # either side of the fused selection's 150 KB: (gx + 2) (gy + 2) <= 7022
    (57, 117, 1, FUSED, 117, 57, 153584), (57, 118, 1, GRID, 118, 57, 118 * 57 * 16),
    # either side of the grid selection's 150 KB: gx gy <= 9600
    (96, 100, 1, GRID, 100, 96, LDS_LIMIT), (96, 101, 1, LIST, 101, 96, 0)])
def test_plan_pins_the_selection_route_and_its_lds(pm, rows, cols, md, route, gx, gy, lds):
    rec = plan(pm, rows, cols, md=md)
    assert (rec["route"], rec["gx"], rec["gy"], rec["select_lds"]) == (route, gx, gy, lds), rec
    assert rec["select_lds"] <= LDS_LIMIT
    # forcing the route it takes anyway gives the same record; a route it can take as well keeps the grid
    assert plan(pm, rows, cols, route, md=md) == rec
    for forced in ROUTES:
        can = forced == LIST or (md >= 1 and (fused_lds(gx, gy) if forced == FUSED else gx * gy * 16) <= LDS_LIMIT)
        if can:
            f = plan(pm, rows, cols, forced, md=md)
            assert (f["route"], f["gx"], f["gy"]) == (forced, gx, gy)
            assert f["select_lds"] == {FUSED: fused_lds(gx, gy), GRID: gx * gy * 16, LIST: 0}[forced]
        else:
            assert refused(pm, rows, cols, forced, md=md), (forced, md)
    assert fused_lds(117, 57) == 153584 and fused_lds(118, 57) > LDS_LIMIT >= fused_lds(64, 36)


def test_plan_pins_the_three_routes_of_the_720p_tests(pm):
    """What tests/test_seed.py::test_sorted_fallback_selection relies on, with its max features."""
    assert [plan(pm, 720, 1280, md=md, maxf=400)["route"] for md in (20, 10, 8)] == [FUSED, GRID, LIST]
    # ... and test_selection_across_many_chunks at 480 x 752: a grid of 3 pixels takes 627 KB, one of 1 pixel 5.7 MB -- only
    # its (300, 40) case runs the fused selection and its chunks, the other two walk the sorted list
    assert [plan(pm, 480, 752, md=md, maxf=mf)["route"] for mf, md in ((1000, 3), (1024, 1), (300, 40))] == [LIST, LIST, FUSED]
    assert plan(pm, 480, 752, md=3)["gx"] * plan(pm, 480, 752, md=3)["gy"] * 16 == 642560


@pytest.mark.parametrize("block, window", [(3, 3), (5, 5), (7, 7), (9, 0), (15, 0), (1, 0), (11, 0)])
def test_plan_pins_the_response_launch(pm, block, window):
    for rows, cols, tx, ty in ((1, 1, 1, 1), (32, 64, 1, 1), (33, 65, 2, 2), (40, 129, 3, 2), (720, 1280, 20, 23)):
        rec = plan(pm, rows, cols, block=block)
        h = block // 2
        assert (rec["response_window"], rec["tiles_x"], rec["tiles_y"]) == (window, tx, ty), rec
        assert rec["response_lds"] == 4 * (64 + 2 * h) * (32 + 2 * h) <= 64 * 1024


def test_plan_pins_the_matcher_lds_and_the_feature_limit(pm):
    assert plan(pm, 240, 376)["match_lds"] == 4 * (11 * 8 + 13 * 33) == 2068        # 31 x 11 template, 128 disparities
    for tc, tr, md in ((5, 3, 17), (6, 3, 18), (7, 5, 19), (8, 1, 20), (9, 9, 9)):
        want = 4 * (tr * ((tc + 3) // 4) + (tr + 2) * ((md + 3) // 4 + 1))
        assert plan(pm, 40, 200, templ_cols=tc, templ_rows=tr, max_disp=md)["match_lds"] == want
    assert [plan(pm, 64, 64, maxf=m)["max_features"] for m in (0, 1, 200, 1024)] == [0, 1, 200, 1024]


def test_plan_refuses_what_a_route_cannot_take(pm):
    for forced in (FUSED, GRID):
        assert refused(pm, 240, 376, forced, md=0) and refused(pm, 240, 376, forced, md=-1)
        assert refused(pm, 32769, 8, forced, md=20) and refused(pm, 8, 32769, forced, md=20)   # x | y << 16 packing
        assert plan(pm, 32768, 8, forced, md=20)["route"] == forced
    assert plan(pm, 32769, 8, md=20)["route"] == LIST and plan(pm, 32769, 8, LIST, md=20)["route"] == LIST
    assert refused(pm, 720, 1280, FUSED, md=10) and refused(pm, 720, 1280, FUSED, md=8) and refused(pm, 720, 1280, GRID, md=8)
    assert refused(pm, 240, 376, 4) and refused(pm, 240, 376, -1)
    assert refused(pm, 0, 376, 0) and refused(pm, 240, 0, 0)
    import ctypes as C
    lib, prm, out = pm.load(), pm.default_params(1), pm.PmDebugSeedPlan()
    assert lib.pm_debug_seed_plan(None, 240, 376, 0, C.byref(out)) == pm.PM_ERR_INVALID_ARG
    assert lib.pm_debug_seed_plan(C.byref(prm), 240, 376, 0, None) == pm.PM_ERR_INVALID_ARG
    out.route = 7
    assert lib.pm_debug_seed_plan(C.byref(prm), 720, 1280, GRID, C.byref(out)) == pm.PM_OK and out.route == GRID
    assert lib.pm_debug_seed_plan(C.byref(prm), 240, 376, 9, C.byref(out)) == pm.PM_ERR_INVALID_ARG and out.route == 0


def test_the_plan_compiles_without_hip_and_walks_its_grid_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/seed_plan_main.cpp: csrc/pm_seed_plan.hpp through g++ (no HIP header in reach) with AddressSanitizer and
    UBSan, over image sizes, min distances, windows, forced routes and the fused switch."""
    import subprocess
    from cpp_build import build_host_kernel
    exe = build_host_kernel(tmp_path / "seed_plan_main", "seed_plan_main.cpp", compiler=("g++",),
                            flags=("-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.endswith(" 0 broken\n"), (r.stdout, r.stderr)


# ---- response, maximum, candidates (pm_debug_seed_trace) ---------------------------------------------------------------------
SHAPES = [(1, 1), (1, 7), (2, 3), (3, 3), (5, 70), (32, 64), (33, 65), (40, 129)]
MAXR, MAXC = 64, 160


def ramp_image(rows, cols):
    return np.tile((np.arange(cols) * 255 // max(cols - 1, 1)).astype(np.uint8), (rows, 1))


def check_response_and_candidates(e, oracle, img, block, harris, k, quality, what):
    t = e.debug_seed_trace(img, img, 2)
    want = oracle.corner_response_map(img, block, harris, k)
    assert np.isfinite(want).all()
    same_bits(t["response"], want, f"response {what}")
    assert t["max_bits"] == seed_ref.max_bits(want), (what, t["max_bits"])
    keys = seed_ref.candidates(want, quality)
    assert t["n_candidates"] == len(keys) == len(t["keys"]), (what, t["n_candidates"], len(keys))
    assert set(t["keys"].tolist()) == keys, what
    if not want.max() > 0:
        assert t["max_bits"] == 0 and t["n_candidates"] == 0 and t["n_accepted"] == 0
    assert t["overflow"] == 0
    return t, want


@pytest.mark.gpu
@pytest.mark.parametrize("block", [3, 5, 7, 9, 15])
@pytest.mark.parametrize("harris, k", [(0, 0.04), (1, 0.04), (1, 0.0)])
def test_response_plane_and_maximum(pm, oracle, block, harris, k):
    """Compiled-in windows and the generic loop; tiles of 64 x 32 with 8 rows per thread; windows wider than the image, where
    reflect-101 loops; Harris responses below zero under a maximum folded on float bits."""
    prm = pm.default_params(1, gftt_block_size=block, gftt_use_harris=harris, gftt_k=k, min_distance_btw_features=2,
                            max_features_per_frame=1024)
    some_negative = False
    with pm.Engine(prm, max_rows=MAXR, max_cols=MAXC) as e:
        for i, (rows, cols) in enumerate(SHAPES):
            _, want = check_response_and_candidates(e, oracle, noise_image(10 + i, rows, cols), block, harris, k, 0.01,
                                                    f"{cols}x{rows} block {block} harris {harris} k {k}")
            some_negative |= bool((want < 0).any())
        # a horizontal ramp: rank-1 tensor everywhere -- Harris below zero at every pixel, the eigenvalue exactly 0
        _, want = check_response_and_candidates(e, oracle, ramp_image(33, 65), block, harris, k, 0.01, "ramp")
        assert want.max() <= 0 and (not (harris and k > 0) or want.max() < 0)
    assert some_negative == bool(harris and k > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind, rows, cols, quality", [("noise", 96, 160, 0.01), ("periodic", 60, 70, 0.01), ("flat", 40, 72, 0.01),
                                                      ("noise", 96, 160, 0.5)])
def test_candidate_keys(pm, oracle, kind, rows, cols, quality):
    img = {"noise": noise_image(1, rows, cols), "periodic": periodic_image(35, rows, cols),
           "flat": np.full((rows, cols), 90, np.uint8)}[kind]
    prm = pm.default_params(1, gftt_quality_level=quality, gftt_block_size=9 if kind == "periodic" else 5)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        t, want = check_response_and_candidates(e, oracle, img, prm.gftt_block_size, 0, 0.04, quality, kind)
        cut = e.debug_seed_trace(img, img, 2, keys_capacity=10)   # a short buffer is not overrun
    print(kind, "candidates:", t["n_candidates"])
    assert len(cut["keys"]) == min(10, t["n_candidates"]) and cut["n_candidates"] == t["n_candidates"]
    if kind == "flat":
        assert t["n_candidates"] == 0
    if kind == "periodic":   # plateaus: neighbouring candidates with EQUAL responses pass the non-strict test together
        ks = sorted(t["keys"].tolist())
        assert any((a >> 32) == (b >> 32) and b - a == 1 for a, b in zip(ks, ks[1:])) or \
               len({k >> 32 for k in ks}) < len(ks) // 4
    if kind == "noise" and quality == 0.01:
        assert t["n_candidates"] > 500


# ---- the selection on synthetic keys, every route (pm_debug_seed_select) -----------------------------------------------------
ROWS, COLS = 150, 260


def size_for(md):
    """The largest of three image sizes at which a grid of md-pixel cells still fits the fused selection's LDS."""
    return (60, 100) if md == 1 else (100, 140) if md == 2 else (ROWS, COLS)


def f32(v):
    return np.float32(v)


def make_keys(seed, n, values, rows=ROWS, cols=COLS, positions=None):
    """n keys at distinct positions (random unless given, [(x, y)]) with the given float32 values, in random order."""
    rng = np.random.default_rng(seed)
    if positions is None:
        flat = rng.choice(rows * cols, n, replace=False)
        positions = [(int(i % cols), int(i // cols)) for i in flat]
    assert len(positions) == n == len(values) and len(set(positions)) == n
    keys = [seed_ref.key_of(v, y, x) for (x, y), v in zip(positions, values)]
    rng.shuffle(keys)
    return np.array(keys, np.uint64)


def uniform_values(seed, n, top=1000.0, quality=0.01):
    """float32 values all over (threshold, top], the maximum among them."""
    thr = float(seed_ref.threshold(top, quality))
    v = np.random.default_rng(seed + 1000).uniform(thr, top, n).astype(np.float32)
    v = np.where(v > f32(thr), v, f32(top))
    if n:
        v[0] = top
    return v


def run_selection(pm, keys, top, md, maxf, quality=0.01, rows=ROWS, cols=COLS, routes=ROUTES):
    """The keys through every route the plan allows -> the list all of them gave, checked against greedy_select."""
    want = seed_ref.greedy_select(keys.tolist(), md, maxf)
    prm = pm.default_params(1, min_distance_btw_features=md, max_features_per_frame=maxf, gftt_quality_level=quality)
    ran = []
    with pm.Engine(prm, max_rows=ROWS, max_cols=COLS) as e:
        for route in (0,) + tuple(routes):
            try:
                pm.seed_plan(prm, rows, cols, route)
            except pm.PmError:
                with pytest.raises(pm.PmError):   # the hook refuses what the plan refuses
                    e.debug_seed_select(keys, int(f32(top).view(np.uint32)), rows, cols, route)
                continue
            xy, overflow = e.debug_seed_select(keys, int(f32(top).view(np.uint32)), rows, cols, route)
            got = [tuple(p) for p in xy.tolist()]
            assert overflow == 0, route
            if got != want:
                first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
                raise AssertionError(f"route {route}: {len(got)} corners, expected {len(want)}; first difference at {first}: "
                                     f"{got[first:first + 3]} vs {want[first:first + 3]}")
            ran.append(route)
    return want, ran


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049, 4100, 5000])
def test_selection_candidate_counts_at_batch_and_chunk_boundaries(pm, n):
    """64-key batches of the greedy loops, 2048-key chunks of the fused selection (its descent starts above 2048 keys)."""
    want, ran = run_selection(pm, make_keys(n, n, uniform_values(n, n)), 1000.0, 3, 1024)
    assert ran == [0, FUSED, GRID, LIST] and len(want) == min(n, len(want)) and (n == 0 or len(want) > 0)
    if n >= 4100:
        assert len(want) == 1024


@pytest.mark.gpu
@pytest.mark.parametrize("maxf", [0, 1, 17, 100, 128, 700, 1024])
def test_selection_feature_limits(pm, maxf):
    """max_features 0, 1, n and the capacity; up to 128 features the fused selection asks for chunks of 512 keys, so its
    descent runs several times over the 5000."""
    n = 700 if maxf == 700 else 5000
    md = 0 if maxf == 700 else 2
    rows, cols = size_for(md)
    want, ran = run_selection(pm, make_keys(7, n, uniform_values(7, n), rows, cols), 1000.0, md, maxf, rows=rows, cols=cols)
    assert len(want) == maxf and ran == ([0, LIST] if md == 0 else [0, FUSED, GRID, LIST])


def _values_case(name):
    n = 3000
    if name == "equal":          # one value: the order is the positions' alone
        return np.full(n, 777.25, np.float32), 777.25, 0.01
    if name == "low_bits":       # values in the lowest mantissa bits below the maximum, quality 0.999: many ties
        top = f32(1.0)
        v = (np.uint32(top.view(np.uint32)) - np.random.default_rng(5).integers(0, 41, n).astype(np.uint32)).view(np.float32)
        v[0] = top
        return v, 1.0, 0.999
    if name == "octaves":        # 20 octaves under quality 1e-6: the first digit of the descent starts high
        v = np.exp2(np.random.default_rng(6).uniform(0.2, 20.0, n)).astype(np.float32)
        v[0] = 2.0 ** 20
        return v, 2.0 ** 20, 1e-6
    if name == "two_levels":     # maximum and threshold share their high bits, the candidates sit at both ends
        v = np.where(np.arange(n) % 2 == 0, f32(1000.0), np.nextafter(f32(999.0), f32(2000.0))).astype(np.float32)
        return v, 1000.0, 0.999
    raise KeyError(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["equal", "low_bits", "octaves", "two_levels"])
@pytest.mark.parametrize("md, maxf", [(3, 1024), (2, 100)])
def test_selection_value_distributions(pm, name, md, maxf):
    """What decides the branches of the fused selection's radix descent: the bits maximum and threshold share, plateaus of
    equal values, values spread over many octaves."""
    v, top, q = _values_case(name)
    assert (v > seed_ref.threshold(top, q)).all() and (v <= f32(top)).all()
    rows, cols = size_for(md)
    want, ran = run_selection(pm, make_keys(11, len(v), v, rows, cols), top, md, maxf, q, rows, cols)
    assert ran == [0, FUSED, GRID, LIST] and len(want) == maxf


@pytest.mark.gpu
@pytest.mark.parametrize("md", [0, -2, 1, 2, 3, 20, 400])
def test_selection_min_distances(pm, md):
    """No min distance (the list alone), 1 .. 20, and one larger than the image's diagonal: a single corner."""
    rows, cols = size_for(md)
    want, ran = run_selection(pm, make_keys(md + 50, 2500, uniform_values(md + 50, 2500), rows, cols), 1000.0, md, 1024,
                              rows=rows, cols=cols)
    assert ran == ([0, LIST] if md < 1 else [0, FUSED, GRID, LIST])
    assert len(want) == (1024 if md <= 1 else 1 if md == 400 else len(want))
    assert md != 20 or 20 < len(want) < 120


@pytest.mark.gpu
@pytest.mark.parametrize("md", [2, 3, 7, 20])
def test_selection_lattices_and_cell_borders(pm, md):
    """Corners exactly md apart keep each other (strict <), corners md - 1 apart do not; points at multiples of md sit on
    cell borders, points in the last row and column in the clamped last cells."""
    rows, cols = size_for(md)
    run = lambda pts, vals, seed: run_selection(pm, make_keys(seed, len(pts), vals, rows, cols, pts), 1000.0, md, 1024,
                                                rows=rows, cols=cols)
    # exactly md: every point is kept, in key order
    pts = [(x, y) for y in range(0, rows, md) for x in range(0, cols, md)]
    pts = pts if len(pts) <= 1024 else [(x, y) for y in range(0, 30 * md, md) for x in range(0, 30 * md, md)]
    want, ran = run(pts, uniform_values(md, len(pts)), md)
    assert len(want) == len(pts) > 100 and ran == [0, FUSED, GRID, LIST]
    # md - 1 along one row, values falling with x: every other point is kept
    step = max(md - 1, 1)
    row = [(x, rows // 2) for x in range(0, cols, step)]
    want, _ = run(row, np.linspace(1000.0, 500.0, len(row)).astype(np.float32), md)
    assert want == row[::2]
    # a lattice of md - 1 across the image, the last row and the last column and the cells' own borders added
    pts = sorted(set([(x, y) for y in range(0, rows, step * 2) for x in range(0, cols, step)][:1500] +
                     [(x, rows - 1) for x in range(0, cols, 2)] + [(cols - 1, y) for y in range(0, rows, 2)] +
                     [(x, y) for y in range(0, rows, md) for x in (0, md, (cols - 1) // md * md - md, (cols - 1) // md * md)]))
    want, ran = run(pts, uniform_values(md + 1, len(pts)), md + 1)
    assert ran == [0, FUSED, GRID, LIST] and len(want) > 10


@pytest.mark.gpu
def test_selection_hook_refuses_what_the_kernels_assume_away(pm):
    prm = pm.default_params(1, min_distance_btw_features=3, max_features_per_frame=1024)
    top = int(f32(1000.0).view(np.uint32))
    with pm.Engine(prm, max_rows=64, max_cols=64) as e:
        ok = make_keys(1, 100, uniform_values(1, 100), 64, 64)
        assert len(e.debug_seed_select(ok, top, 64, 64)[0]) > 0
        for bad in (seed_ref.key_of(1000.0, 64, 3), seed_ref.key_of(1000.0, 3, 64),       # outside the image
                    seed_ref.key_of(1001.0, 3, 3), seed_ref.key_of(10.0, 3, 3),          # above the maximum, at the threshold
                    seed_ref.key_of(float("nan"), 3, 3), seed_ref.key_of(-5.0, 3, 3)):
            with pytest.raises(pm.PmError) as err:
                e.debug_seed_select(np.append(ok, np.uint64(bad)), top, 64, 64)
            assert err.value.status == pm.PM_ERR_INVALID_ARG and "pm_debug_seed_select" in str(err.value)
        with pytest.raises(pm.PmError) as err:   # beyond the scratch: 64 rows x 64 + 64 slots
            e.debug_seed_select(np.zeros(64 * 64 + 65, np.uint64), top, 64, 64)
        assert err.value.status == pm.PM_ERR_INVALID_ARG
        with pytest.raises(pm.PmError) as err:
            e.debug_seed_select(ok, top, 65, 64)
        assert err.value.status == pm.PM_ERR_SIZE


@pytest.mark.gpu
@pytest.mark.parametrize("maxf", [1024, 17])
def test_detector_through_every_route_equals_the_oracle(pm, oracle, maxf):
    """The noise image at 150 x 260 through the trace: candidates, then each route's selection, == oracle.gftt_detect; fewer
    features give a prefix."""
    img = noise_image(2, ROWS, COLS)
    prm = pm.default_params(1, min_distance_btw_features=3, max_features_per_frame=maxf)
    sp = oracle.seed_params(min_distance=3, max_features=maxf)
    xs, ys = oracle.gftt_detect(img, sp)
    full = oracle.gftt_detect(img, oracle.seed_params(min_distance=3, max_features=1024))
    assert np.array_equal(xs, full[0][:maxf]) and np.array_equal(ys, full[1][:maxf]) and len(xs) == maxf
    with pm.Engine(prm, max_rows=ROWS, max_cols=COLS) as e:
        for route in (0,) + ROUTES:
            t = e.debug_seed_trace(img, np.roll(img, -5, axis=1), 2, route)
            assert t["n_candidates"] > 2048 and t["overflow"] == 0
            assert np.array_equal(t["xy"], np.stack([xs, ys], axis=1)), route
            assert np.array_equal(t["xy_rounded"], t["xy"]) and t["xy_f"] is None


# ---- the matcher on corners at every border (pm_debug_seed_match) ------------------------------------------------------------
def oracle_matches(oracle, left, right, xy, sp, xy_f=None):
    kx = xy[:, 0].astype(np.float32) if xy_f is None else xy_f[:, 0]
    ky = xy[:, 1].astype(np.float32) if xy_f is None else xy_f[:, 1]
    return np.array([oracle.match_rectified(left, right, float(x), float(y), sp) for x, y in zip(kx, ky)], np.float32)


def row_and_column(rows, cols, y, x):
    return np.array([(i, y) for i in range(cols)] + [(x, j) for j in range(rows)], np.int32)


def shifted_noise_pair(seed, rows, cols, shift):
    right = noise_image(seed, rows, cols)
    return np.roll(right, shift, axis=1), right


def check_matches(e, oracle, left, right, xy, sp, what, xy_f=None):
    got = e.debug_seed_match(left, right, xy, xy_f)
    want = oracle_matches(oracle, left, right, xy, sp, xy_f)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {bad.size} of {len(xy)} corners differ; first: corner {xy[bad[0]].tolist()} device " \
                          f"{got[bad[0]]!r} oracle {want[bad[0]]!r}"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("tc, tr, md", [(5, 3, 17), (6, 3, 18), (7, 5, 19), (8, 1, 20), (9, 9, 9), (31, 11, 128)])
def test_matcher_at_every_border(pm, oracle, tc, tr, md):
    """Every x of one row and every y of one column of a 40 x 200 pair shifted by 7: templates clipped at the left and
    right border, stripes clamped at both ends, templates and stripes leaving the image vertically; template widths of
    every residue mod 4, disparity ranges that are no multiple of 4."""
    rows, cols = 40, 200
    left, right = shifted_noise_pair(4, rows, cols, 7)
    xy = row_and_column(rows, cols, 20, 100)
    prm = pm.default_params(1, templ_cols=tc, templ_rows=tr, max_disp=md)
    sp = oracle.seed_params(templ_cols=tc, templ_rows=tr, max_disp=md)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        got = check_matches(e, oracle, left, right, xy, sp, f"template {tc}x{tr}, {md} disparities")
        # corners outside the image and far from it match nothing and fault nothing
        far = np.array([(-1, 20), (cols, 20), (100, -1), (100, rows), (-5000, 20), (100, 70000), (2 ** 20, -2 ** 20)], np.int32)
        out = check_matches(e, oracle, left, right, far, sp, "corners outside")
        assert (out[2:] == -1).all() and (md - tc < 7 or out[1] == 7)   # (a corner rounded to `cols` still has its template)
        assert len(e.debug_seed_match(left, right, np.zeros((0, 2), np.int32))) == 0
    if md - tc >= 7:   # the stripe reaches a disparity of md - tc: the shift is found, and nothing else is
        assert set(np.unique(got).tolist()) == {-1.0, 7.0}
    if (tc, tr, md) == (31, 11, 128):   # the branches the inputs are meant to reach, spelled out for the default template
        by_x, by_y = got[:cols], got[cols:]
        assert (by_x[:22] == -1).all() and (by_x[22:] == 7).all()
        assert (by_y[:6] == -1).all() and (by_y[6:33] == 7).all() and (by_y[33:] == -1).all()
    if md == tc:                        # one position per stripe row, disparity 0: found on an identical pair only
        with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
            assert (check_matches(e, oracle, right, right, xy, sp, "identical pair") == 0).any()


@pytest.mark.gpu
def test_matcher_ties_denominators_and_refusals(pm, oracle):
    rows, cols = 40, 200
    prm = pm.default_params(1, templ_cols=7, templ_rows=3, max_disp=40)
    sp = oracle.seed_params(templ_cols=7, templ_rows=3, max_disp=40)
    xy = row_and_column(rows, cols, 20, 100)
    noise = noise_image(8, rows, cols)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        # a pair of period 6: the cost is exactly 0 at every sixth position -- the first minimum wins
        per = periodic_image(3, rows, cols, 5, 6)
        got = check_matches(e, oracle, per, per, xy, sp, "periodic pair")
        inner = got[60:140]
        assert (inner == 30).all()   # zeros at 0, 6 .. 30 of the 34 positions: the leftmost one, the largest disparity
        # a black right image: the denominator vanishes, the cost is 1, nothing matches
        got = check_matches(e, oracle, noise, np.zeros_like(noise), xy, sp, "black right image")
        assert (got == -1).all()
        got = check_matches(e, oracle, np.zeros_like(noise), np.zeros_like(noise), xy, sp, "black pair")
        assert (got == -1).all()
        # unrelated images: a best cost far above max_matching_cost
        assert (check_matches(e, oracle, noise, noise_image(9, rows, cols), xy, sp, "unrelated images") == -1).mean() > 0.9
        # the swapped pair: the best match lies to the right and is refused; the shifted one is found
        left, right = shifted_noise_pair(4, rows, cols, 7)
        assert (check_matches(e, oracle, left, right, xy, sp, "shifted pair") == 7).any()
        assert not (check_matches(e, oracle, right, left, xy, sp, "swapped pair") == 7).any()
        # identical images: disparity 0 is a match
        assert (check_matches(e, oracle, noise, noise, xy, sp, "identical pair") == 0).any()
    # at 64 x 96 the default 128 disparities are more than the image holds: nothing matches, as such
    p64 = shifted_noise_pair(5, 64, 96, 7)
    with pm.Engine(pm.default_params(1), max_rows=64, max_cols=96) as e:
        got = check_matches(e, oracle, p64[0], p64[1], row_and_column(64, 96, 30, 50), oracle.seed_params(), "64x96")
        assert (got == -1).all()
        for bad in (np.array([[2 ** 20 + 1, 3]]), np.array([[3, -2 ** 20 - 1]])):
            with pytest.raises(pm.PmError) as err:
                e.debug_seed_match(p64[0], p64[1], bad)
            assert err.value.status == pm.PM_ERR_INVALID_ARG and "pm_debug_seed_match" in str(err.value)


@pytest.mark.gpu
def test_matcher_with_subpixel_refinement(pm, oracle, synth):
    """subpixel_refinement with sub-pixel corners: the matcher compares the corner's own x with the refined match."""
    rows, cols = 96, 200
    p = synth.make_pair(7, rows=rows, cols=cols)
    kw = dict(templ_cols=21, templ_rows=7, max_disp=64, subpixel_refinement=1)
    sp = oracle.seed_params(**kw)
    xs, ys = oracle.gftt_detect(p["left"], oracle.seed_params(min_distance=6, max_features=150))
    rng = np.random.default_rng(3)
    xy_f = (np.stack([xs, ys], axis=1) + rng.choice([-0.375, -0.25, 0.125, 0.25, 0.3125], (len(xs), 2))).astype(np.float32)
    xy = np.floor(xy_f + np.float32(0.5)).astype(np.int32)   # roundf: no fraction above is a half
    with pm.Engine(pm.default_params(1, **kw), max_rows=rows, max_cols=cols) as e:
        got = check_matches(e, oracle, p["left"], p["right"], xy, sp, "sub-pixel corners", xy_f)
        plain = check_matches(e, oracle, p["left"], p["right"], xy, sp, "integer corners")
    ok = got >= 0
    assert ok.sum() > 10 and not np.all(got[ok] == np.rint(got[ok])) and not np.array_equal(got, plain)


# ---- the splat on corners an image would not produce (pm_debug_seed_splat) -----------------------------------------------------
def splat_corners(rows, cols):
    """Corners with d = -1, 0 and > 0; duplicates, later ones with d = 0 and d = -1 among them; corners rounded to -1 and to
    cols / rows; rectangles clipped at all four borders and corners."""
    c = [(0, 0, 5.0), (cols - 1, 0, 6.5), (0, rows - 1, 7.0), (cols - 1, rows - 1, 8.0), (cols // 2, 0, 3.0),
         (cols // 2, rows - 1, 4.0), (0, rows // 2, 9.0), (cols - 1, rows // 2, 2.5),
         (20, 12, 11.0), (21, 13, 12.0), (40, 12, -1.0), (41, 12, 0.0), (42, 20, 0.5),
         (-1, 10, 30.0), (cols, 10, 31.0), (10, -1, 32.0), (10, rows, 33.0), (-1, -1, 34.0),
         (30, 25, 20.0), (30, 25, 10.0),                 # a duplicate with a smaller value behind
         (50, 25, 10.0), (50, 25, 20.0),                 # ... with a larger value behind
         (60, 28, 15.0), (60, 28, 0.0),                  # ... with d = 0 behind: valid, owns the pixel
         (15, 30, 16.0), (15, 30, -1.0),                 # ... with d = -1 behind: does not count
         (35, 30, 17.0), (35, 30, -1.0), (35, 30, 13.0), (35, 30, 0.0), (35, 30, 14.0), (35, 30, -1.0)]
    return np.array([(x, y) for x, y, _ in c], np.int32), np.array([d for _, _, d in c], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 2, 17])
@pytest.mark.parametrize("dedup", [0, 1])
def test_splat(pm, k, dedup):
    rows, cols = 37, 75            # rows no multiple of 4: the last group of a state plane is partial
    xy, d = splat_corners(rows, cols)
    with pm.Engine(pm.default_params(1), max_rows=40, max_cols=80) as e:
        for inv in (1.0, 0.25):
            want = seed_ref.splat(xy, d, rows, cols, k, inv, bool(dedup))
            for layout in (0, 1):
                same_bits(e.debug_seed_splat(xy, d, rows, cols, k, inv, dedup, None, layout), want,
                          f"k {k} dedup {dedup} scale {inv} layout {layout}")
        assert not e.debug_seed_splat(xy[:0], d[:0], rows, cols, k).any()            # no corner: the memset alone
        only_bad = d <= 0
        assert not e.debug_seed_splat(xy[only_bad], d[only_bad], rows, cols, k, 1.0, dedup, None, 1).any()
    assert (want > 0).any() and (k == 17 or (want == 0).any())
    if dedup:
        assert want[25, 30] == 10.0 * 0.25 or k > 0


@pytest.mark.gpu
@pytest.mark.parametrize("out_shape", [(39, 65), (119, 197), (59, 98), (1, 1)])
def test_splat_with_resize(pm, oracle, out_shape):
    """119 x 197 -> 39 x 65: sizes that do not divide (Initialize with f = 3), both layouts."""
    rows, cols = 119, 197
    rng = np.random.default_rng(12)
    xy = np.stack([rng.integers(-2, cols + 2, 300), rng.integers(-2, rows + 2, 300)], axis=1).astype(np.int32)
    xy[250:] = xy[200:250]   # duplicates
    d = rng.choice(np.array([-1.0, 0.0, 0.5, 3.0, 17.0, 40.25, 127.0], np.float32), 300)
    with pm.Engine(pm.default_params(1), max_rows=rows, max_cols=cols) as e:
        for k, inv, dedup in ((5, 0.125, 1), (2, 1.0, 0), (3, 0.25, 1)):
            want = seed_ref.splat(xy, d, rows, cols, k, inv, bool(dedup), out_shape)
            for layout in (0, 1):
                same_bits(e.debug_seed_splat(xy, d, rows, cols, k, inv, dedup, out_shape, layout), want,
                          f"{out_shape} k {k} scale {inv} dedup {dedup} layout {layout}")
    assert want.shape == out_shape and (out_shape == (1, 1) or ((want > 0).any() and (want == 0).any()))


@pytest.mark.gpu
def test_splat_hook_refusals_and_the_capture_rule(pm):
    xy, d = splat_corners(37, 75)
    with pm.Engine(pm.default_params(1), max_rows=40, max_cols=80) as e:
        for kw in (dict(k=-1), dict(dedup=2), dict(state_layout=2), dict(out_shape=(38, 75)), dict(inv_scale=0.0)):
            args = dict(rows=37, cols=75, k=2)
            args.update(kw)
            with pytest.raises(pm.PmError) as err:
                e.debug_seed_splat(xy, d, **args)
            assert err.value.status == pm.PM_ERR_INVALID_ARG and "pm_debug_seed_splat" in str(err.value), kw
        with pytest.raises(pm.PmError) as err:
            e.debug_seed_splat(xy, np.where(d == 0.5, np.float32("nan"), d), 37, 75, 2)
        assert "NaN" in str(err.value)
        # between pm_capture_begin and pm_capture_end every seeder hook is refused: a recorded Match() around the refused
        # calls, as tests/test_noise_cost.py captures it
        import torch
        img = noise_image(1, 37, 75)
        before = e.debug_seed_splat(xy, d, 37, 75, 2)
        t = lambda a: torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda:0"))
        L, S = t(img), t(np.zeros((37, 75), np.float32))
        DL, DR = torch.empty_like(S), torch.empty_like(S)
        run = lambda: e.match_device(1, L.data_ptr(), L.data_ptr(), 37, 75, S.data_ptr(), S.data_ptr(), DL.data_ptr(),
                                     DR.data_ptr())
        run()
        e.synchronize()
        e.capture_begin()
        for call in (lambda: e.debug_seed_splat(xy, d, 37, 75, 2), lambda: e.debug_seed_trace(img, img, 2),
                     lambda: e.debug_seed_match(img, img, xy), lambda: e.debug_seed_select(np.zeros(0, np.uint64), 0, 37, 75)):
            with pytest.raises(pm.PmError) as err:
                call()
            assert err.value.status == pm.PM_ERR_BUSY and "pm_debug_seed_" in str(err.value)
        run()
        e.capture_end()
        e.replay()
        e.synchronize()
        same_bits(e.debug_seed_splat(xy, d, 37, 75, 2), before, "after the capture")


# ---- the whole trace against the oracle's composition ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(subpixel_corners=1, subpix_winsize=5, subpixel_refinement=1)])
def test_trace_names_every_stage_of_a_scene(pm, oracle, synth, kw):
    """Every intermediate result of one pm_sparse_init equals the oracle's, and the parts compose to pm_sparse_init's map."""
    rows, cols = 133, 259
    p = synth.make_pair(3, rows=rows, cols=cols)
    l, r = p["left"], p["right"]
    sp = oracle.seed_params(min_distance=9, **kw)
    with pm.Engine(pm.default_params(1, min_distance_btw_features=9, **kw), max_rows=rows, max_cols=cols) as e:
        t = e.debug_seed_trace(l, r, 3)
        whole = e.sparse_init(l, r, 3)
    resp = oracle.corner_response_map(l, sp.block_size, 0, sp.harris_k)
    same_bits(t["response"], resp, "response")
    assert set(t["keys"].tolist()) == seed_ref.candidates(resp, sp.quality_level)
    xs, ys = oracle.gftt_detect(l, sp)
    assert np.array_equal(t["xy"], np.stack([xs, ys], axis=1)) and t["overflow"] == 0
    fx, fy = xs.astype(np.float32), ys.astype(np.float32)
    if kw:
        fx, fy = oracle.corner_subpix(l, fx, fy, sp.subpix_winsize, sp.subpix_zerozone, sp.subpix_maxiters, sp.subpix_epsilon)
        assert np.array_equal(bits(t["xy_f"]), bits(np.stack([fx, fy], axis=1)))
    rounded = np.stack([np.floor(np.abs(fx) + np.float32(0.5)) * np.sign(fx), np.floor(np.abs(fy) + np.float32(0.5)) * np.sign(fy)],
                       axis=1).astype(np.int32)
    assert np.array_equal(t["xy_rounded"], rounded)
    d = np.array([oracle.match_rectified(l, r, float(x), float(y), sp) for x, y in zip(fx, fy)], np.float32)
    assert np.array_equal(bits(t["d"]), bits(d)) and (d > 0).any()
    same_bits(t["seed"], seed_ref.splat(rounded, d, rows, cols, 2 ** 3 + 1), "seed map from the parts")
    same_bits(t["seed"], oracle.sparse_init(l, r, 3, sp), "seed map")
    same_bits(whole, t["seed"], "pm_sparse_init")
