"""The stages of the row-tiled phase API (pm_tile_*, csrc/pm_tile.hip), one launch at a time, against the oracle.

tests/test_tiled.py holds the tiled MAP to the untiled one; pm_tile_finish returns owned rows only, so a stage that writes
halo rows, a column restore that forgets the cost plane, a masked sweep that also sweeps unflagged columns or an exchange
round whose mask is too wide all end in the right map.  Here every test has ONE band on ONE handle: state goes in through
the seeds, pm_tile_set_row and pm_debug_tile_state, comes out through pm_debug_tile_state (include/pm/testing.h), and is
compared with tests/tile_ref.py -- the whole-image oracle stage restricted to the owned rows -- at tolerance 0, in BOTH
state planes of BOTH views, over the WHOLE band: cells a stage must not write hold sentinels, the cost plane included.

The first two tests prove the reference itself on the CPU: bands chained in sweep order reproduce the whole-image sweep.
"""
import collections
import functools

import numpy as np
import pytest

import noise_cost_ref
import tile_ref
from conftest import assert_same

SEM_CPU, SEM_GPU = 0, 1
ENGINE_SERIAL, ENGINE_WAVE, ENGINE_RUN = 1, 2, 5      # PM_ENGINE_* (include/pm/patchmatch.h)
K_TILE_ROUND_ROWS = 16                                # csrc/pm_kernels.hpp::kTileRoundRows
# The cost plane of every cell a stage must not write: larger than any cost, so that a sweep that strays into such a row
# adopts its predecessor's value there and shows in BOTH planes (below every cost it would never adopt and stay unseen).
COST_SENTINEL = np.float32(1e30)
WINDOWS = [(11, 11), (5, 5), (7, 3)]                  # (patch_h, patch_w)


def assert_bits(got, want, what):
    """assert_same on the bit patterns: an untouched cell keeps its bits, and no +0 / -0 confusion passes."""
    assert_same(np.asarray(got, np.float32).view(np.uint32), np.asarray(want, np.float32).view(np.uint32), what)


# ---- the definition, on the CPU --------------------------------------------------------------------------------------------
CHAIN_BANDS = [(0, 17), (17, 18), (18, 20), (20, 41), (41, 61)]   # [first owned row, end)


@functools.lru_cache(maxsize=8)
def pair_views(rows, cols, index=71):
    import oracle_lib
    import synth
    p = synth.make_pair(index, rows=rows, cols=cols, n_points=max(40, rows * cols // 300), dilate_factor=3)
    return tile_ref.view_images(oracle_lib, p["left"], p["right"]), p["seed_l"], p["seed_r"]


def random_map(rng, rows, cols, hi=30.0):
    """finite values >= 0, a third of them background, some of them too large for their column (the clamp)"""
    d = rng.uniform(0, hi, (rows, cols)).astype(np.float32)
    d[rng.random((rows, cols)) < 0.33] = 0
    return d


@pytest.mark.parametrize("sem,window", [(SEM_CPU, w) for w in WINDOWS] + [(SEM_GPU, (3, 3))])
@pytest.mark.parametrize("view", [0, 1])
def test_bands_chained_in_sweep_order_are_the_whole_column_sweep(oracle, sem, window, view):
    """tile_ref.column_sweep over the bands [0,17) [17,18) [18,20) [20,41) [41,61) of a 61 x 96 pair, downwards in order
    and upwards in reverse order, equals the oracle's sweep of the whole image -- also for the bands that hold the first
    rows, the last rows and (PM_SEM_GPU) the trimmed far end -- and no crop changes a row outside its band (asserted
    inside column_sweep)."""
    ph, pw = window
    rows, cols = 61, 96
    images = pair_views(rows, cols)[0][view]
    d = random_map(np.random.default_rng(5 + view), rows, cols)
    for k in (1, 3):
        want = tile_ref.whole_sweep(oracle, sem, images, d, ph, pw, k)
        assert (want != d).mean() > 0.05, "a sweep that adopts nothing proves nothing"
        got = d
        for a, end in (CHAIN_BANDS if k == 1 else CHAIN_BANDS[::-1]):
            got = tile_ref.column_sweep(oracle, sem, images, got, a, end - 1, ph, pw, k)
        assert_bits(got, want, f"semantics {sem} window {ph}x{pw} view {view} sweep {k}: bands in order vs whole image")
        # ... and out of order they are NOT: the predecessor row matters (the reference is sensitive to it)
        stale = d
        for a, end in (CHAIN_BANDS[::-1] if k == 1 else CHAIN_BANDS):
            stale = tile_ref.column_sweep(oracle, sem, images, stale, a, end - 1, ph, pw, k)
        assert not np.array_equal(stale, want)


@pytest.mark.parametrize("sem,ph", [(SEM_CPU, 11), (SEM_CPU, 5), (SEM_CPU, 7), (SEM_GPU, 3)])
def test_crop_geometry_matches_the_rows_the_whole_sweep_visits(sem, ph):
    """crop_rows / swept_rows against the loops of the reference restated: for every band [a, b] of a 24-row image the
    crop's first and last processed rows are the first and last owned rows the whole-image sweep visits, and the
    predecessor row lies inside the crop."""
    G = 24
    for a in range(G):
        for b in range(a, G):
            for k in (1, 3):
                if sem == SEM_CPU:
                    whole = list(range(ph // 2, G - ph // 2))
                else:
                    whole = list(range(1, G - 2)) if k == 1 else list(range(G - 2, 1, -1))
                mine = [y for y in (whole if k == 1 or sem == SEM_GPU else whole[::-1]) if a <= y <= b]
                c0, c1 = tile_ref.crop_rows(sem, G, a, b, ph, k)
                h = c1 - c0 + 1
                if sem == SEM_CPU:
                    crop = [c0 + y for y in range(max(ph // 2, 1 if k == 1 else 0), min(h - ph // 2, h if k == 1 else h - 1))]
                    crop = crop if k == 1 else crop[::-1]
                else:
                    crop = [c0 + y for y in (range(1, h - 2) if k == 1 else range(h - 2, 1, -1))]
                assert crop == mine, (a, b, k, crop, mine)
                rows = tile_ref.swept_rows(sem, G, a, b, ph, k)
                assert rows == ((mine[0], mine[-1]) if mine else None), (a, b, k)
                if mine:
                    pred = mine[0] - 1 if k == 1 else mine[0] + 1
                    assert c0 <= pred <= c1, (a, b, k)


# ---- one band on one handle ----------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu
G = 64                                                # rows of the whole image of most cases
Geom = collections.namedtuple("Geom", "G band0 band_rows own0 own_rows")
REQUIRED_OWN_ROWS = {1, 2, 3, K_TILE_ROUND_ROWS - 1, K_TILE_ROUND_ROWS, K_TILE_ROUND_ROWS + 1, 2 * K_TILE_ROUND_ROWS + 1}


def make_geom(halo, own0, own_rows, band0_mod=None, rows=G):
    """The band of owned rows [own0, own0 + own_rows) with the halo pm_tile_begin wants; band0_mod: the remainder mod 4
    its first row shall have, reached by a WIDER halo at the top, which pm_tile_begin accepts.  A band has 8 rows and more
    (check_size), so a short one near an image border takes a wider halo as well."""
    need_top, end = max(own0 - halo, 0), min(own0 + own_rows + halo, rows)
    band0 = need_top
    if band0_mod is not None and need_top - ((need_top - band0_mod) % 4) >= 0:
        band0 = need_top - ((need_top - band0_mod) % 4)
    while end - band0 < 8:
        if end < rows:
            end += 1
        else:
            band0 -= 1
    return Geom(rows, band0, end - band0, own0, own_rows)


def band_geometries(sem, ph, rows=G):
    """Top, middle and bottom bands; every remainder mod 4 of the band's first row and of the owned offset; owned rows
    around kTileRoundRows and below k_runblk3's shortest segment; bands outside and partly outside the interior."""
    halo = tile_ref.halo_rows(sem, [ph])
    n_out = ph // 2 if sem == SEM_CPU else 1     # rows above (and below) the interior
    t = [(0, 17, None), (17, 1, 3), (18, 2, 1), (20, 3, 1), (23, 15, 2), (25, 16, 1), (31, 33, 3), (47, 17, 2),
         (0, n_out, None), (rows - n_out, n_out, 0),                      # wholly outside the interior
         (n_out - 1, 4, None), (rows - n_out - 2, n_out + 2, 2)]          # partly
    return [make_geom(halo, own0, own_rows, mod, rows) for own0, own_rows, mod in t]


@pytest.mark.parametrize("sem,ph", [(SEM_CPU, 11), (SEM_CPU, 5), (SEM_CPU, 7), (SEM_GPU, 3)])
def test_the_geometries_cover_what_they_claim(sem, ph):
    halo = tile_ref.halo_rows(sem, [ph])
    gs = band_geometries(sem, ph)
    lo, hi = tile_ref.interior_rows(sem, G, ph)
    for g in gs:
        assert 0 <= g.band0 <= max(g.own0 - halo, 0) and g.band0 + g.band_rows >= min(g.own0 + g.own_rows + halo, G)
        assert g.band0 + g.band_rows <= G and g.band_rows >= 8
    assert {g.band0 % 4 for g in gs} == {0, 1, 2, 3}
    assert {(g.own0 - g.band0) % 4 for g in gs} == {0, 1, 2, 3}
    assert REQUIRED_OWN_ROWS <= {g.own_rows for g in gs}
    assert any(g.band0 < max(g.own0 - halo, 0) for g in gs), "a wider halo than needed"
    assert any(g.own0 == 0 for g in gs) and any(g.own0 + g.own_rows == G for g in gs)
    assert any(g.band0 > 0 and g.band0 + g.band_rows < G for g in gs)
    outside = [g for g in gs if g.own0 + g.own_rows - 1 < lo or g.own0 > hi]
    partly = [g for g in gs if (g.own0 < lo <= g.own0 + g.own_rows - 1) or (g.own0 <= hi < g.own0 + g.own_rows - 1)]
    assert len(outside) >= 2 and len(partly) >= 2, (outside, partly)


def make_params(pm, sem, window, engine=0, iters=1, amp=None, bg=None, views=2):
    ph, pw = window if sem == SEM_CPU else (3, 3)
    bh, bw = (bg or window) if sem == SEM_CPU else (3, 3)
    kw = dict(patchmatch_iters=iters, engine=engine, left_right_check=int(views == 2), patch_h=[ph] * iters,
              patch_w=[pw] * iters, bg_patch_h=bh, bg_patch_w=bw)
    if amp is not None:
        kw["noise_amp"] = [amp] * iters
    return pm.default_params(sem, **kw)


class Band:
    """One open band: the images of its rows on the device, pm_tile_begin without seeds, state in and out."""

    def __init__(self, pm, e, g, cols, views):
        import torch
        self.pm, self.e, self.g, self.cols, self.views = pm, e, g, cols, views
        self.device = torch.device("cuda:0")
        self.kept = []
        (v0, _), _, _ = pair_views(g.G, cols)
        rows = slice(g.band0, g.band0 + g.band_rows)
        self.images = [self.up(v0[0][rows]), self.up(v0[1][rows])]
        e.tile_begin(pm.PmTile(g.G, g.band0, g.own0, g.own_rows), self.images[0].data_ptr(), self.images[1].data_ptr(),
                     g.band_rows, cols, None, None)
        self.a, self.b = g.own0, g.own0 + g.own_rows - 1
        self.own = np.zeros(g.band_rows, bool)
        self.own[g.own0 - g.band0:g.own0 - g.band0 + g.own_rows] = True

    def up(self, a):
        """A device copy that lives as long as the band: the stages read it on the handle's stream, not on torch's."""
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.kept.append(t)
        return t

    def write(self, states):
        for v, (d, c) in enumerate(states):
            self.e.debug_tile_state_write(v, d, c)

    def read(self, which=0):
        return [self.e.debug_tile_state((self.g.band_rows, self.cols), which, v) for v in range(self.views)]

    def set_row(self, image_row, rows):
        """rows: [views][cols] -> pm_tile_set_row"""
        t = self.up(np.asarray(rows, np.float32))
        self.e.tile_set_row(image_row, t.data_ptr())
        self.e.synchronize()

    def band_rows_of(self, whole):
        return whole[self.g.band0:self.g.band0 + self.g.band_rows]


@functools.lru_cache(maxsize=None)
def raw_map(rows, cols, view):
    d = random_map(np.random.default_rng(11 + view), rows, cols)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def base_state(sem, window, rows, cols, view):
    """(disp, cost) of a whole image in the state a sweep finds: disp a random map, clamped where PM_SEM_CPU's noise + cost
    stage clamps; cost the cost of disp in the interior, the sentinel everywhere else.  From tests/noise_cost_ref.py."""
    import oracle_lib as O
    ph, pw = window
    sentinel = np.full((rows, cols), COST_SENTINEL, np.float32)
    ims = O.ImageSet(*pair_views(rows, cols)[0][view])
    disp, cost = noise_cost_ref.stage(O, ims, sem, raw_map(rows, cols, view), pw, ph, -1.0, 0, None, sentinel)
    disp, cost = np.ascontiguousarray(disp, np.float32), np.ascontiguousarray(cost, np.float32)
    disp.setflags(write=False)
    cost.setflags(write=False)
    return disp, cost


def band_input(band, sem, window):
    """per view (disp, cost) of the band's rows of base_state; the cost plane of the rows it does not own: the sentinel"""
    out = []
    for v in range(band.views):
        D, Cst = base_state(sem, window, band.g.G, band.cols, v)
        d, c = band.band_rows_of(D).copy(), band.band_rows_of(Cst).copy()
        c[~band.own] = COST_SENTINEL
        out.append((d, c))
    return out


def check_band(band, got, before, want_own, what):
    """got / before: [(disp, cost)] per view over the whole band; want_own: per view (disp, cost) of the owned rows.
    Owned rows equal the reference, every other row keeps its bits, in both planes."""
    for v in range(band.views):
        for i, plane in enumerate(("disparity", "cost")):
            assert_bits(got[v][i][band.own], want_own[v][i], f"{what}: view {v} {plane} plane, owned rows")
            assert_bits(got[v][i][~band.own], before[v][i][~band.own], f"{what}: view {v} {plane} plane, rows NOT owned")


def whole_images(rows, cols, view):
    return pair_views(rows, cols)[0][view]


# ---- noise + clamp + cost ------------------------------------------------------------------------------------------------------
ROW_LOCAL_CASES = [(SEM_CPU, (11, 11), 150, 2), (SEM_CPU, (5, 5), 47, 1), (SEM_CPU, (7, 3), 150, 2), (SEM_GPU, (3, 3), 150, 2),
                   (SEM_GPU, (3, 3), 47, 1)]


@gpu
@pytest.mark.parametrize("sem,window,cols,views", ROW_LOCAL_CASES)
def test_noise_stage_of_a_band(pm, oracle, sem, window, cols, views):
    """pm_tile_noise with a real amplitude: both planes of the owned rows equal the whole-image stage (the band's slice of
    the whole-image noise table, the Sobel rows of the minimal halo, the clamp, the cost), every other row of both planes
    keeps its bits -- the halo rows hold the neighbours' values, positive ones among them."""
    ph, pw = window
    amp = 4.0
    params = make_params(pm, sem, window, amp=amp, views=views)
    with pm.Engine(params, max_rows=G, max_cols=cols) as e:
        unit = e.unit_noise(G, cols)
        assert np.abs(unit[G // 2:]).max() > 0.5
        sentinel = np.full((G, cols), COST_SENTINEL, np.float32)
        want = [noise_cost_ref.stage(oracle, oracle.ImageSet(*whole_images(G, cols, v)), sem, raw_map(G, cols, v), pw, ph, amp,
                                     0, unit, sentinel) for v in range(views)]
        for g in band_geometries(sem, ph):
            band = Band(pm, e, g, cols, views)
            before = [(band.band_rows_of(raw_map(G, cols, v)).copy(), band.band_rows_of(sentinel).copy()) for v in range(views)]
            band.write(before)
            e.tile_noise(0)
            got = band.read()
            check_band(band, got, before, [(w[0][band.a:band.b + 1], w[1][band.a:band.b + 1]) for w in want], f"noise, {g}")
        with pytest.raises(pm.PmError) as err:
            e.tile_noise(1)
        assert err.value.status == pm.PM_ERR_INVALID_ARG


# ---- row sweeps, background, finish ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def row_stage_reference(sem, window, bg, cols, view, factor):
    """whole image: [(disp, cost) after the row +1 sweep, after the row -1 sweep, after the background mask]"""
    import oracle_lib as O
    ph, pw = window
    images = whole_images(G, cols, view)
    d0, c0 = base_state(sem, window, G, cols, view)
    out = []
    d, c = d0, c0
    for k in (0, 2):
        d2 = tile_ref.whole_sweep(O, sem, images, d, ph, pw, k)
        c2 = tile_ref.cost_after(O, sem, images, pw, ph, d, c, d2)
        out.append((d2, c2))
        d, c = d2, c2
    ims = O.ImageSet(*images)
    if sem == SEM_CPU:
        d3 = O.cpu_remove_background(ims, d, bg[0], bg[1], factor=factor, nthreads=4)
    else:
        d3 = O.gpu_mask_background(ims, d, improve=factor, nthreads=4)
    out.append((d3, c))
    return out


@gpu
@pytest.mark.parametrize("sem,window,cols,views", ROW_LOCAL_CASES + [(SEM_CPU, (11, 11, 5, 5), 150, 2)])
def test_row_sweeps_background_and_finish_of_a_band(pm, oracle, sem, window, cols, views):
    """pm_tile_sweep k = 0, 2, pm_tile_background (the cached window, and -- the last case: iterations 11 x 11, background
    5 x 5 -- a window the cost plane does not belong to) and pm_tile_finish, one after the other on every geometry."""
    import torch
    window, bg = window[:2], (window[2:] or window[:2])
    ph, pw = window
    params = make_params(pm, sem, window, bg=bg, views=views)
    factor = float(params.win_by_factor if sem == SEM_CPU else params.cost_improve_factor)
    refs = [row_stage_reference(sem, window, bg, cols, v, factor) for v in range(views)]
    with pm.Engine(params, max_rows=G, max_cols=cols) as e:
        for g in band_geometries(sem, max(ph, bg[0])):
            band = Band(pm, e, g, cols, views)
            before = band_input(band, sem, window)
            band.write(before)
            own = slice(band.a, band.b + 1)
            for stage, call in enumerate((lambda: e.tile_sweep(0, 0), lambda: e.tile_sweep(0, 2), e.tile_background)):
                call()
                got = band.read()
                check_band(band, got, before, [(r[stage][0][own], r[stage][1][own]) for r in refs],
                           f"{('row +1 sweep', 'row -1 sweep', 'background')[stage]}, {g}")
                if stage < 2:
                    rec = e.debug_tile_last_sweep()
                    lo, hi = tile_ref.interior_rows(sem, G, ph)
                    chains = max(min(hi, band.b) - max(lo, band.a) + 1, 0)
                    assert (rec["axis"], rec["dir"], rec["chains"]) == ((0, 1 - 2 * stage, chains) if chains else (0, 0, 0)), (g, rec)
            # finish: the cross-check of the owned rows, nothing behind them, and the band is closed
            n = g.own_rows * cols
            outs = [torch.full((n + cols,), -5.0, dtype=torch.float32, device=band.device) for _ in range(views)]
            e.tile_finish(outs[0].data_ptr(), outs[1].data_ptr() if views > 1 else None)
            e.synchronize()
            dl = got[0][0][band.own]
            if views > 1:
                dr = np.ascontiguousarray(got[1][0][band.own][:, ::-1])
                assert_bits(outs[1].cpu().numpy()[:n].reshape(-1, cols), dr, f"finish, right map, {g}")
                dl = oracle.gpu_mask_occlusions(dl, dr)
            assert_bits(outs[0].cpu().numpy()[:n].reshape(-1, cols), dl, f"finish, left map, {g}")
            for o in outs:
                assert (o.cpu().numpy()[n:] == -5.0).all(), f"finish wrote behind the owned rows, {g}"
            for call in (lambda: e.tile_noise(0), lambda: e.tile_sweep(0, 0), e.tile_background,
                         lambda: e.debug_tile_state((g.band_rows, cols))):
                with pytest.raises(pm.PmError) as err:
                    call()
                assert err.value.status == pm.PM_ERR_INVALID_ARG and "pm_tile_begin" in str(err.value)


# ---- column sweeps ---------------------------------------------------------------------------------------------------------------
def pred_row_of(band, k):
    """the image row in front of the band's chains of column sweep k, None: the image ends there"""
    r = band.a - 1 if k == 1 else band.b + 1
    return r if 0 <= r < band.g.G else None


def column_case(band, sem, window, k, seed):
    """(pred, new_rows, before, want): the predecessor row and what pm_tile_set_row puts there -- values the whole-image
    sweep would NOT have left --, the band's planes in front of the sweep, and the owned rows behind it (tile_ref)."""
    import oracle_lib as O
    ph, pw = window
    g, own = band.g, slice(band.a, band.b + 1)
    pred = pred_row_of(band, k)
    new_rows = random_map(np.random.default_rng(seed), band.views, band.cols)
    before, want = [], []
    for v in range(band.views):
        D, Cst = base_state(sem, window, g.G, band.cols, v)
        images = whole_images(g.G, band.cols, v)
        W = D.copy()
        if pred is not None:
            assert not np.array_equal(W[pred], new_rows[v])
            W[pred] = new_rows[v]
        after = tile_ref.column_sweep(O, sem, images, W, band.a, band.b, ph, pw, k)
        cost = tile_ref.cost_after(O, sem, images, pw, ph, W, Cst, after)
        d, c = band.band_rows_of(W).copy(), band.band_rows_of(Cst).copy()
        c[~band.own] = COST_SENTINEL
        before.append((d, c))
        want.append((after[own], cost[own]))
    return pred, new_rows, before, want


def run_waves(chain_len, chains_in_launch):
    """plan_sweep's rule (csrc/pm_sweep_plan.hpp): wavefronts per chain of the run engine"""
    return 8 if chain_len > 1600 else 2 if (chain_len < 400 and chains_in_launch >= 2048) else 4


def check_record(rec, band, sem, window, engine, k, what):
    """pm_debug_tile_last_sweep after column sweep k: the engine (no chain of a band is beyond the LDS), the axis, the
    direction, chain_len = the owned rows the whole-image sweep visits, the chains, the wavefronts per chain."""
    ph, pw = window
    rows = tile_ref.swept_rows(sem, band.g.G, band.a, band.b, ph, k)
    if rows is None:
        assert not any(rec.values()), (what, rec)
        return
    chain_len = abs(rows[1] - rows[0]) + 1
    chains = band.cols - (pw - 1) if sem == SEM_CPU else band.cols - 2
    assert (rec["engine"], rec["axis"], rec["dir"], rec["chain_len"], rec["chains"]) == \
        (engine, 1, 1 if k == 1 else -1, chain_len, chains), (what, rec)
    assert rec["waves"] == (run_waves(chain_len, chains * band.views) if engine == ENGINE_RUN else 0), (what, rec)


ENGINES = (ENGINE_SERIAL, ENGINE_WAVE, ENGINE_RUN)
COLUMN_CASES = [(SEM_CPU, w, eng, 150, 2) for w in WINDOWS for eng in ENGINES] + \
               [(SEM_GPU, (3, 3), eng, 150, 2) for eng in ENGINES] + \
               [(SEM_CPU, (11, 11), ENGINE_RUN, 47, 1), (SEM_GPU, (3, 3), ENGINE_RUN, 47, 1)]


@gpu
@pytest.mark.parametrize("sem,window,engine,cols,views", COLUMN_CASES)
def test_column_sweeps_of_a_band(pm, sem, window, engine, cols, views):
    """pm_tile_sweep k = 1, 3 on every geometry: the chains start in the middle of the state planes, behind a predecessor
    row that pm_tile_set_row filled; owned rows equal the crop reference in both planes, the predecessor row and every
    other row keep their bits, and the record shows what was launched (4 wavefronts per chain at these sizes)."""
    params = make_params(pm, sem, window, engine=engine, views=views)
    with pm.Engine(params, max_rows=G, max_cols=cols) as e:
        for i, g in enumerate(band_geometries(sem, window[0])):
            band = Band(pm, e, g, cols, views)
            for k in (1, 3):
                what = f"semantics {sem} window {window} engine {engine} sweep {k}, {g}"
                pred, new_rows, before, want = column_case(band, sem, window, k, 100 * i + k)
                band.write(band_input(band, sem, window))
                if pred is not None:
                    band.set_row(pred, new_rows)
                e.tile_sweep(0, k)
                rec = e.debug_tile_last_sweep()
                check_band(band, band.read(), before, want, what)
                check_record(rec, band, sem, window, engine, k, what)
                if engine == ENGINE_RUN and any(rec.values()):
                    assert rec["waves"] == 4, (what, rec)


@gpu
@pytest.mark.parametrize("sem,window", [(SEM_CPU, (11, 11)), (SEM_GPU, (3, 3))])
def test_column_sweeps_of_a_wide_band_take_two_wavefronts_per_chain(pm, sem, window):
    """40 x 1040, two views, owned rows [6, 28): chains of 22 positions in a launch of more than 2048 chains -- the
    waves = 2 variant of plan_sweep, which a band otherwise meets only at 4096 x 2160."""
    rows, cols, views = 40, 1040, 2
    params = make_params(pm, sem, window, engine=ENGINE_RUN, views=views)
    g = make_geom(tile_ref.halo_rows(sem, [window[0]]), 6, 22, rows=rows)
    with pm.Engine(params, max_rows=rows, max_cols=cols) as e:
        band = Band(pm, e, g, cols, views)
        for k in (1, 3):
            what = f"semantics {sem} window {window} sweep {k}, {g}"
            pred, new_rows, before, want = column_case(band, sem, window, k, k)
            band.write(band_input(band, sem, window))
            band.set_row(pred, new_rows)
            e.tile_sweep(0, k)
            rec = e.debug_tile_last_sweep()
            check_band(band, band.read(), before, want, what)
            check_record(rec, band, sem, window, ENGINE_RUN, k, what)
            assert (rec["waves"], rec["chain_len"]) == (2, 22), (what, rec)


# ---- the masked column sweep --------------------------------------------------------------------------------------------------
def column_masks(sem, window, cols, views, rng):
    """name -> [views][cols] int32; a flag is any non-zero value"""
    pw = window[1]
    lo, hi = (pw // 2, cols - pw // 2 - 1) if sem == SEM_CPU else (1, cols - 2)
    zero = np.zeros((views, cols), np.int32)
    one = zero.copy()
    one[0, 70] = 1
    one[-1, 5] = 1
    border = zero.copy()
    border[:, :lo] = 1
    border[:, hi + 1:] = 1
    half = (rng.random((views, cols)) < 0.5).astype(np.int32) * 3
    first = zero.copy()
    first[0] = -1           # view 0: every column, view 1: none
    return {"none": zero, "all": zero + 7, "one column": one, "border columns": border, "random half": half,
            "view 0 only": first}


def masked(mask_row, flagged, unflagged):
    return np.where(mask_row[None, :] != 0, flagged, unflagged)


MASKED_CASES = [(SEM_CPU, w, eng) for w in ((11, 11), (7, 3)) for eng in ENGINES] + [(SEM_CPU, (5, 5), ENGINE_RUN)] + \
               [(SEM_GPU, (3, 3), eng) for eng in ENGINES]


@gpu
@pytest.mark.parametrize("sem,window,engine", MASKED_CASES)
def test_masked_column_sweeps_of_a_band(pm, sem, window, engine):
    """pm_tile_sweep_masked: the flagged columns equal the unmasked sweep, the others keep their bits in both planes; the
    mask path (chain_active, csrc/pm_device.hpp) of every engine under both semantics; refused for k = 0, 2 and without
    a mask."""
    cols, views = 150, 2
    params = make_params(pm, sem, window, engine=engine, views=views)
    gs = band_geometries(sem, window[0])
    with pm.Engine(params, max_rows=G, max_cols=cols) as e:
        for i in (1, 3, 4, 6):      # 1, 3 and 15 owned rows in the middle, 33 at the bottom
            band = Band(pm, e, gs[i], cols, views)
            for k in (1, 3):
                pred, new_rows, before, want = column_case(band, sem, window, k, 100 * i + k)
                full = [(before[v][0].copy(), before[v][1].copy()) for v in range(views)]   # the unmasked sweep's planes
                for v in range(views):
                    for p in range(2):
                        full[v][p][band.own] = want[v][p]
                for name, mask in column_masks(sem, window, cols, views, np.random.default_rng(i)).items():
                    what = f"semantics {sem} window {window} engine {engine} sweep {k} mask '{name}', {gs[i]}"
                    band.write(band_input(band, sem, window))
                    if pred is not None:
                        band.set_row(pred, new_rows)
                    d_mask = band.up(mask)
                    e.tile_sweep_masked(0, k, d_mask.data_ptr())
                    rec = e.debug_tile_last_sweep()
                    got = band.read()
                    for v in range(views):
                        for p, plane in enumerate(("disparity", "cost")):
                            assert_bits(got[v][p], masked(mask[v], full[v][p], before[v][p]), f"{what}: view {v} {plane} plane")
                    check_record(rec, band, sem, window, engine, k, what)
        d_mask = band.up(np.ones((views, cols), np.int32))
        before = band.read()
        for call in (lambda: e.tile_sweep_masked(0, 0, d_mask.data_ptr()), lambda: e.tile_sweep_masked(0, 2, d_mask.data_ptr()),
                     lambda: e.tile_sweep_masked(0, 1, None), lambda: e.tile_sweep_masked(0, 4, d_mask.data_ptr())):
            with pytest.raises(pm.PmError) as err:
                call()
            assert err.value.status == pm.PM_ERR_INVALID_ARG
            assert not any(e.debug_tile_last_sweep().values())
        after = band.read()
        for v in range(views):
            for p in range(2):
                assert_bits(after[v][p], before[v][p], "a refused masked sweep changed the state")


# ---- snapshot, presweep, restore, restore_cols ----------------------------------------------------------------------------------
def random_planes(rng, band):
    """per view (disp, cost): any finite values, every cell another one -- these stages only move them"""
    shape = (band.g.band_rows, band.cols)
    return [(rng.uniform(0, 40, shape).astype(np.float32), rng.uniform(0, 60, shape).astype(np.float32))
            for _ in range(band.views)]


def assert_planes(got, want, what):
    for v, (g, w) in enumerate(zip(got, want)):
        for p, plane in enumerate(("disparity", "cost")):
            assert_bits(g[p], w[p], f"{what}: view {v} {plane} plane")


@gpu
@pytest.mark.parametrize("cols,views", [(150, 2), (47, 1)])
def test_snapshot_presweep_restore_and_restore_cols(pm, cols, views):
    """pm_tile_presweep(row) = pm_tile_set_row + pm_tile_snapshot in both the live and the snapshot planes, with the
    predecessor row in every remainder mod 4 of the interleaved state planes; with a null row the snapshot alone;
    pm_tile_restore brings both planes back; pm_tile_restore_cols exactly the flagged columns of both planes."""
    params = make_params(pm, SEM_CPU, (5, 5), views=views)
    rng = np.random.default_rng(cols)
    g = make_geom(3, 21, 18, 1)                   # rows 17 .. 41, owned 21 .. 38
    assert g.band_rows % 4 != 0                   # the last four-row piece of the planes is a partial one
    with pm.Engine(params, max_rows=G, max_cols=cols) as e:
        band = Band(pm, e, g, cols, views)
        with pytest.raises(pm.PmError) as err:    # no snapshot yet on this handle
            band.read(which=1)
        assert err.value.status == pm.PM_ERR_INVALID_ARG
        for call in (e.tile_restore, lambda: e.tile_restore_cols(band.up(np.ones((views, cols), np.int32)).data_ptr())):
            with pytest.raises(pm.PmError) as err:
                call()
            assert err.value.status == pm.PM_ERR_INVALID_ARG and "snapshot" in str(err.value)
        s0 = random_planes(rng, band)
        band.write(s0)
        e.tile_snapshot()
        assert_planes(band.read(1), s0, "pm_tile_snapshot: the snapshot")
        assert_planes(band.read(0), s0, "pm_tile_snapshot: the live planes")
        rows = [g.band0, g.band0 + 1, g.own0 - 1, g.own0 + g.own_rows, g.band0 + g.band_rows - 1, g.own0 + 5]
        assert {(r - g.band0) % 4 for r in rows} == {0, 1, 2, 3}
        for r in rows:
            s0 = random_planes(rng, band)
            band.write(s0)
            row = rng.uniform(0, 40, (views, cols)).astype(np.float32)
            e.tile_presweep(r, band.up(row).data_ptr())
            want = [(d.copy(), c) for d, c in s0]
            for v in range(views):
                want[v][0][r - g.band0] = row[v]
            assert_planes(band.read(0), want, f"pm_tile_presweep(row {r}): the live planes")
            assert_planes(band.read(1), want, f"pm_tile_presweep(row {r}): the snapshot")
        s1 = random_planes(rng, band)
        band.write(s1)
        e.tile_presweep(g.own0 - 1, None)         # the snapshot alone
        assert_planes(band.read(0), s1, "pm_tile_presweep(null): the live planes")
        assert_planes(band.read(1), s1, "pm_tile_presweep(null): the snapshot")
        with pytest.raises(pm.PmError) as err:
            e.tile_presweep(g.band0 + g.band_rows, band.up(row).data_ptr())
        assert err.value.status == pm.PM_ERR_INVALID_ARG
        s2 = random_planes(rng, band)
        band.write(s2)
        assert_planes(band.read(1), s1, "writing the live planes moved the snapshot")
        masks = column_masks(SEM_CPU, (5, 5), cols, views, rng) if cols == 150 else \
            {"random half": (rng.random((views, cols)) < 0.5).astype(np.int32), "none": np.zeros((views, cols), np.int32)}
        for name, mask in masks.items():
            band.write(s2)
            e.tile_restore_cols(band.up(mask).data_ptr())
            want = [tuple(masked(mask[v], s1[v][p], s2[v][p]) for p in range(2)) for v in range(views)]
            assert_planes(band.read(0), want, f"pm_tile_restore_cols, mask '{name}'")
            assert_planes(band.read(1), s1, f"pm_tile_restore_cols, mask '{name}': the snapshot")
        band.write(s2)
        e.tile_restore()
        assert_planes(band.read(0), s1, "pm_tile_restore")
        # the hook's own refusals
        for which, view, write in ((2, 0, 0), (0, views, 0), (0, -1, 0), (1, 0, 1)):
            rc = e.lib.pm_debug_tile_state(e.h, which, view, None, None, write)
            assert rc == pm.PM_ERR_INVALID_ARG, (which, view, write)
    with pm.Engine(params, max_rows=G, max_cols=cols) as e:     # without an open band
        assert e.lib.pm_debug_tile_state(e.h, 0, 0, None, None, 0) == pm.PM_ERR_INVALID_ARG
        assert not any(e.debug_tile_last_sweep().values())


# ---- one exchange round ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sem,window,engine", [(SEM_CPU, (11, 11), ENGINE_RUN), (SEM_CPU, (5, 5), ENGINE_SERIAL),
                                               (SEM_GPU, (3, 3), ENGINE_RUN), (SEM_GPU, (3, 3), ENGINE_WAVE)])
def test_exchange_round_is_restore_cols_set_row_and_masked_sweep(pm, sem, window, engine):
    """pm_tile_exchange_round against its definition, composed from the stages the tests above hold to the oracle:
    both planes of both views equal pm_tile_restore_cols(incoming != used) + pm_tile_set_row + pm_tile_sweep_masked,
    d_mask is exactly incoming != used per view, used_next equals incoming -- also where it IS incoming -- and owned rows
    of 1, 15, 16, 17 and 33 around kTileRoundRows."""
    cols, views = 150, 2
    params = make_params(pm, sem, window, engine=engine, views=views)
    gs = band_geometries(sem, window[0])
    with pm.Engine(params, max_rows=G, max_cols=cols) as e:
        for i in (1, 4, 5, 7, 6):
            band = Band(pm, e, gs[i], cols, views)
            for k in (1, 3):
                pred = pred_row_of(band, k)
                if pred is None:
                    continue
                what = f"semantics {sem} window {window} engine {engine} sweep {k}, {gs[i]}"
                rng = np.random.default_rng(10 * i + k)
                used = random_map(rng, views, cols)
                incoming = used.copy()
                changed = np.zeros((views, cols), bool)
                changed[0, [0, 63, 64, cols - 1]] = True
                changed[0] |= rng.random(cols) < 0.2
                changed[1] = rng.random(cols) < 0.3
                changed[1, [0, cols - 1]] = False
                incoming[changed] += np.float32(1.5)

                def first_sweep():
                    band.write(band_input(band, sem, window))
                    e.tile_presweep(pred, band.up(used).data_ptr())
                    e.tile_sweep(0, k)

                results = []
                for alias in (False, True):
                    first_sweep()
                    d_in, d_used = band.up(incoming), band.up(used)
                    d_next = d_in if alias else band.up(np.full((views, cols), -1.0, np.float32))
                    d_mask = band.up(np.full((views, cols), 9, np.int32))
                    e.tile_exchange_round(0, k, pred, d_in.data_ptr(), d_used.data_ptr(), d_next.data_ptr(), d_mask.data_ptr())
                    rec = e.debug_tile_last_sweep()
                    e.synchronize()
                    assert np.array_equal(d_mask.cpu().numpy(), changed.astype(np.int32)), f"{what}: d_mask (alias {alias})"
                    assert_bits(d_next.cpu().numpy(), incoming, f"{what}: used_next (alias {alias})")
                    assert_bits(d_used.cpu().numpy(), used, f"{what}: used")
                    check_record(rec, band, sem, window, engine, k, what)
                    results.append(band.read())
                first_sweep()
                d_mask = band.up(changed.astype(np.int32))
                e.tile_restore_cols(d_mask.data_ptr())
                band.set_row(pred, incoming)
                e.tile_sweep_masked(0, k, d_mask.data_ptr())
                want = band.read()
                assert_planes(results[0], want, f"{what}: exchange round vs its three stages")
                assert_planes(results[1], want, f"{what}: exchange round with used_next = incoming vs its three stages")
                # ... and the columns whose incoming value did not change are those of the first sweep
                first_sweep()
                once = band.read()
                for v in range(views):
                    for p in range(2):
                        assert_bits(want[v][p][:, ~changed[v]], once[v][p][:, ~changed[v]], f"{what}: unflagged columns")
        # the documented refusals (the band of 33 rows at the bottom is open, a snapshot exists)
        d_row, d_mask = band.up(used), band.up(np.zeros((views, cols), np.int32))
        d_next = band.up(used)
        bad = [(1, band.a, d_next), (1, band.b, d_next), (0, band.a - 1, d_next), (2, band.a - 1, d_next),
               (1, band.a - 1, d_row), (1, band.g.band0 - 1, d_next)]
        for k, row, nxt in bad:
            with pytest.raises(pm.PmError) as err:
                e.tile_exchange_round(0, k, row, d_row.data_ptr(), d_row.data_ptr(), nxt.data_ptr(), d_mask.data_ptr())
            assert err.value.status == pm.PM_ERR_INVALID_ARG, (k, row)
            assert not any(e.debug_tile_last_sweep().values())


# ---- did a boundary row move? --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cols,views", [(150, 2), (47, 1)])
def test_row_moved_flag(pm, cols, views):
    """pm_tile_row_moved: the flag stays 0 on equal rows whatever the other rows hold, becomes 1 for ONE differing element
    -- at column 0, 63, 64 or cols - 1, in the last view only --, and a flag that is set stays set."""
    params = make_params(pm, SEM_CPU, (5, 5), views=views)
    rng = np.random.default_rng(cols)
    g = make_geom(3, 21, 18, 1)
    with pm.Engine(params, max_rows=G, max_cols=cols) as e:
        band = Band(pm, e, g, cols, views)
        state = random_planes(rng, band)
        band.write(state)
        for r in (g.own0, g.own0 + g.own_rows - 1, g.band0, g.own0 + 2):
            ref = np.stack([state[v][0][r - g.band0] for v in range(views)])

            def moved(row, preset=0):
                flag = band.up(np.array([preset], np.int32))
                e.tile_row_moved(r, band.up(row).data_ptr(), flag.data_ptr())
                e.synchronize()
                return int(flag.cpu().numpy()[0])

            assert moved(ref) == 0, f"row {r}: equal rows"
            assert moved(ref, preset=1) == 1, f"row {r}: a set flag stays set"
            for x in sorted({0, 63, 64, cols - 1} & set(range(cols))):
                other = ref.copy()
                other[views - 1, x] += np.float32(0.25)
                assert moved(other) == 1, f"row {r}: one element differs at column {x} of view {views - 1}"
            # other rows do not matter
            noisy = [(d.copy(), c.copy()) for d, c in state]
            for v in range(views):
                keep = noisy[v][0][r - g.band0].copy()
                noisy[v][0][:] += np.float32(1)
                noisy[v][0][r - g.band0] = keep
                noisy[v][1][:] += np.float32(1)
            band.write(noisy)
            assert moved(ref) == 0, f"row {r}: only other rows differ"
            band.write(state)
        flag = band.up(np.zeros(1, np.int32))
        for row in (g.band0 - 1, g.band0 + g.band_rows):
            with pytest.raises(pm.PmError) as err:
                e.tile_row_moved(row, band.up(ref).data_ptr(), flag.data_ptr())
            assert err.value.status == pm.PM_ERR_INVALID_ARG


# ---- pm_tile_begin's geometry checks ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sem,window", [(SEM_CPU, (11, 11)), (SEM_CPU, (7, 3)), (SEM_GPU, (3, 3))])
def test_begin_refuses_bands_that_do_not_hold_their_halo(pm, sem, window):
    """The halo rule: max_ph / 2 + 1 rows (PM_SEM_GPU: 2) of image data on both sides of the owned rows, clipped to the
    image.  (global_rows, band_row0, band_rows, own_row0, own_rows, accepted)"""
    import torch
    cols = 47
    halo = tile_ref.halo_rows(sem, [window[0]])
    assert halo == {(SEM_CPU, 11): 6, (SEM_CPU, 7): 4, (SEM_GPU, 3): 2}[sem, window[0]]
    table = [(G, 20 - halo, 10 + 2 * halo, 20, 10, True),           # exactly the halo
             (G, 20 - halo - 3, 10 + 2 * halo + 5, 20, 10, True),   # more
             (G, 20 - halo + 1, 10 + 2 * halo - 1, 20, 10, False),  # one row short at the top
             (G, 20 - halo, 10 + 2 * halo - 1, 20, 10, False),      # ... at the bottom
             (G, 0, 10 + halo, 0, 10, True),                        # clipped at the top of the image
             (G, G - 10 - halo, 10 + halo, G - 10, 10, True),       # ... and at its bottom
             (G, G - 10 - halo, 11 + halo, G - 10, 10, False),      # the band ends behind the image
             (G, 40, 20, 50, 15, False),                            # the owned rows do
             (G, 20 - halo, 2 * halo + 8, 20, 0, False),            # no owned row
             (G, 20 - halo, 2 * halo + 8, 20, -1, False),
             (G, -1, 30, 0, 10, False),
             (G, 20 - halo, 10 + 2 * halo, -1, 10, False)]
    params = make_params(pm, sem, window, views=1)
    dev = torch.device("cuda:0")
    img = torch.zeros((G, cols), dtype=torch.uint8, device=dev)
    with pm.Engine(params, max_rows=G, max_cols=cols) as e:
        for rows, band0, band_rows, own0, own_rows, ok in table:
            call = lambda: e.tile_begin(pm.PmTile(rows, band0, own0, own_rows), img.data_ptr(), img.data_ptr(), band_rows, cols,
                                        None, None)
            if ok:
                call()
                assert e.debug_tile_state((band_rows, cols))[0].shape == (band_rows, cols)
            else:
                with pytest.raises(pm.PmError) as err:
                    call()
                assert err.value.status == pm.PM_ERR_INVALID_ARG and "pm_tile_begin" in str(err.value), (band0, band_rows, own0, own_rows)
        e.synchronize()


# ---- the stages in order, by hand -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sem,patch", [(SEM_CPU, 11), (SEM_GPU, 3)])
def test_stages_driven_by_hand_equal_the_untiled_match(pm, oracle, sem, patch):
    """The pipelined schedule over the bands [0,17) [17,18) [18,20) [20,40) -- one, two and three owned rows among them,
    which no driver produces -- three iterations with the default noise: in a column sweep the bands take turns along the
    sweep direction, each behind its predecessor's final boundary row.  Equal to Match() on the whole pair and to the
    oracle."""
    import torch
    rows, cols, iters = 40, 96, 3
    (v0, _), sl, sr = pair_views(rows, cols)
    left, right = v0[0], v0[1]
    params = pm.default_params(sem, patch=patch, patchmatch_iters=iters)
    halo = tile_ref.halo_rows(sem, [patch])
    bounds = [(0, 17), (17, 18), (18, 20), (20, 40)]
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    engines, geoms, keep = [], [], []
    try:
        for a, end in bounds:
            g = make_geom(halo, a, end - a, rows=rows)
            e = pm.Engine(params, max_rows=max(g.band_rows, 16), max_cols=cols)
            engines.append(e)
            geoms.append(g)
            s = slice(g.band0, g.band0 + g.band_rows)
            t = [up(left[s]), up(right[s]), up(sl[s]), up(sr[s])]
            keep.append(t)
            e.tile_begin(pm.PmTile(rows, g.band0, g.own0, g.own_rows), t[0].data_ptr(), t[1].data_ptr(), g.band_rows, cols,
                         t[2].data_ptr(), t[3].data_ptr())
        row = torch.empty((2, cols), dtype=torch.float32, device=dev)
        for it in range(iters):
            for e in engines:
                e.tile_noise(it)
            for k in range(4):
                if k in (0, 2):
                    for e in engines:
                        e.tile_sweep(it, k)
                    continue
                order = range(len(engines)) if k == 1 else range(len(engines) - 1, -1, -1)
                for pos, i in enumerate(order):
                    e, g = engines[i], geoms[i]
                    if pos > 0:
                        e.tile_set_row(g.own0 - 1 if k == 1 else g.own0 + g.own_rows, row.data_ptr())
                    e.tile_sweep(it, k)
                    e.tile_get_row(g.own0 + g.own_rows - 1 if k == 1 else g.own0, row.data_ptr())
                    e.synchronize()
        dl, dr = np.empty((rows, cols), np.float32), np.empty((rows, cols), np.float32)
        for e, g in zip(engines, geoms):
            e.tile_background()
            out = [torch.empty((g.own_rows, cols), dtype=torch.float32, device=dev) for _ in range(2)]
            e.tile_finish(out[0].data_ptr(), out[1].data_ptr())
            e.synchronize()
            dl[g.own0:g.own0 + g.own_rows] = out[0].cpu().numpy()
            dr[g.own0:g.own0 + g.own_rows] = out[1].cpu().numpy()
    finally:
        for e in engines:
            e.close()
    with pm.Engine(params, max_rows=rows, max_cols=cols) as e:
        ul, ur = e.match(left, right, sl, sr)
    assert_same(dl, ul, "stages by hand vs untiled Match (left)")
    assert_same(dr, ur, "stages by hand vs untiled Match (right)")
    el, er = oracle.match(oracle.default_params(sem, patch=patch, n_iters=iters, nthreads=8), left, right, sl, sr)
    assert_same(dl, el, "stages by hand vs oracle (left)")
    assert_same(dr, er, "stages by hand vs oracle (right)")
    assert (dl > 0).mean() > 0.05
