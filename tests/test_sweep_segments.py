"""Segment boundaries of the run engine on the device: every hint source on every sweep direction, against the oracle.

k_runblk3 cuts a chain into (64 / group) * waves segments (csrc/pm_run3.hpp).  Where the segments begin is the equal split
or, with a hint, balanced by predicted stops (csrc/pm_seg_bounds.hpp); the fix-up rounds end at the sequential sweep either
way, so EVERY hint -- garbage included -- must give the oracle's map at tolerance 0.  pm_debug_propagate_hinted
(include/pm/testing.h) selects the hint source per pass, hands the row +1 pass a stop-bit plane and returns the boundaries
one chain used, which are compared with pm_debug_segment_bounds, the header function (tests/test_segment_bounds.py pins
that one on the host).

Shapes: chains just below, at and above nseg * 8 positions, the shortest chain that takes a hint --
  4 wavefronts (the default bucket): 8 / 16 segments of 32 / 16 lanes: 64 and 128 positions -> 54, 64, 65, 128, 138;
  2 wavefronts (chains shorter than 400 in launches of 2048 chains or more): 4 / 8 segments: 32 and 64 -> 31 .. 33, 63 .. 65;
  8 wavefronts (chains longer than 1600): 16 / 32 segments; nseg * 8 = 128 / 256 lies far below 1600, so that bucket is
  covered above its boundary only, by chains of 1690 positions.
Every shape has at least six chains: rows (columns) of every remainder mod 4 of the interleaved state planes.
"""
import functools

import numpy as np
import pytest

import sweep_fields
from conftest import assert_same

pytestmark = pytest.mark.gpu

SEM_CPU, ENGINE_RUN = 0, 5
NONE, RUNS, PLANE = 0, 1, 2
AMP_G16, AMP_G32 = 0.25, 1e30      # 16- / 32-lane groups for window 11 (tests/test_sweep_variants.py)
MIN_LEN = 8


def shape_of(axis, pw, n, chains):
    along, across = n + pw - 1, chains + pw - 1
    return (across, along) if axis == 0 else (along, across)


@functools.lru_cache(maxsize=8)
def images(pw, axis, rows, cols):
    l, r, d = sweep_fields.one_value_runs(pw, "rows" if axis == 0 else "cols", rows, cols)
    return l, r, d


def field(kind, pw, axis, rows, cols):
    """-> (left, right, disparity).  constant: nothing ever stops; noise: every position a stop; head / tail: noise on the
    first / last eighth of every chain and one value elsewhere -- all predicted stops crowd at one end; runs: one value
    that runs through whole segments (tests/sweep_fields.py): the fix-up cascade and the wide step."""
    l, r, runs = images(pw, axis, rows, cols)
    rng = np.random.default_rng(99)
    noise = rng.uniform(1.0, 30.0, (rows, cols)).astype(np.float32)
    if kind == "runs":
        return l, r, runs
    if kind == "constant":
        return l, r, np.full((rows, cols), sweep_fields.RUN_VALUE, np.float32)
    if kind == "noise":
        return l, r, noise
    d = np.full((rows, cols), sweep_fields.RUN_VALUE, np.float32)
    length = cols if axis == 0 else rows
    cut = max(length // 8, pw // 2 + 3)
    sel = slice(0, cut) if kind == "head" else slice(length - cut, length)
    if axis == 0:
        d[:, sel] = noise[:, sel]
    else:
        d[sel, :] = noise[sel, :]
    return l, r, d


def chain_values(m, pw, axis, direction, chain):
    """the values of chain `chain` (image row / column) in sweep order, with the pixel before the chain in front"""
    h = pw // 2
    line = m[chain, :] if axis == 0 else m[:, chain]
    inner = line[h - 1:len(line) - h] if direction > 0 else line[::-1][h - 1:len(line) - h]
    return inner


def check_case(pm, oracle, pw, axis, n, chains, kinds, amps, expect_waves):
    rows, cols = shape_of(axis, pw, n, chains)
    passes = (0, 2) if axis == 0 else (1, 3)
    prm = pm.default_params(SEM_CPU, patch=3, patchmatch_iters=1, engine=ENGINE_RUN)
    rng = np.random.default_rng(rows * 7 + cols)
    chain = pw // 2 + min(3, chains - 1)      # an interior row / column
    hinted_seen = 0
    with pm.Engine(prm, max_rows=rows, max_cols=cols, max_batch=1) as e:
        for kind in kinds:
            l, r, d = field(kind, pw, axis, rows, cols)
            ims = oracle.ImageSet(l, r)
            # the state the sweeps start from: the map after the stage's clamp, no pass
            start = e.debug_propagate_hinted(l, r, d, pw, pw, 0)[0]
            for k in passes:
                direction = 1 if k < 2 else -1
                want = oracle.cpu_propagate(ims, d, pw, pw, pass_mask=1 << k, nthreads=8)
                planes = {"none": None}
                if k == 0:
                    true = np.zeros((rows, cols), np.uint8)
                    true[:, 1:] = want[:, 1:] != want[:, :-1]
                    planes = {"zeros": np.zeros((rows, cols), np.uint8), "ones": np.full((rows, cols), 255, np.uint8),
                              "random": (rng.random((rows, cols)) < 0.3).astype(np.uint8), "true": true}
                for amp in amps:
                    for mode in (NONE, RUNS, PLANE):
                        for pname, plane in (planes.items() if mode == PLANE else [("none", None)]):
                            hints = [NONE] * 4
                            hints[k] = mode
                            what = f"window {pw} axis {axis} n {n} chains {chains} {kind} pass {k} amp {amp} hint {mode} plane {pname}"
                            got, recs, stops, bounds = e.debug_propagate_hinted(l, r, d, pw, pw, 1 << k, amp, hints,
                                                                                stops=plane, bounds_of=(k, chain))
                            assert_same(got, want, what)
                            rec = recs[0]
                            assert rec["engine"] == ENGINE_RUN and rec["chain_len"] == n and rec["waves"] == expect_waves, (what, rec)
                            nseg = (64 // rec["group"]) * rec["waves"]
                            nd = rec["group"] - pw + (1 if axis == 1 else 0)
                            # the boundaries the kernel used are the header function's for the flags it was given
                            if mode == RUNS:
                                v = chain_values(start, pw, axis, direction, chain)
                                flags = (v[1:] != v[:-1]).astype(np.uint8)
                            elif mode == PLANE and k == 0 and plane is not None:
                                h = pw // 2
                                flags = plane[chain, h:cols - h]
                            else:
                                flags = None
                            assert flags is None or flags.shape == (n,), what
                            assert bounds == pm.segment_bounds(flags, n, nseg, nd), (what, bounds)
                            if flags is not None and flags.any() and n >= nseg * MIN_LEN:
                                hinted_seen += 1
                                assert all(b1 - b0 >= MIN_LEN for b0, b1 in zip(bounds, bounds[1:])), (what, bounds)
                            if k == 0 and plane is not None:
                                # the row +1 pass wrote its stop bits: interior pixels, 1 where the value changes
                                h = pw // 2
                                assert np.array_equal(stops[h:rows - h, h:cols - h], planes["true"][h:rows - h, h:cols - h]), what
    return hinted_seen


ALL_KINDS = ("constant", "noise", "head", "tail", "runs")
DEFAULT_CASES = [(pw, axis, n) for pw in (11, 5) for axis in (0, 1) for n in (54, 64, 65, 128, 138)]


@pytest.mark.parametrize("pw, axis, n", DEFAULT_CASES)
def test_four_wavefronts_around_the_shortest_hinted_chain(pm, oracle, pw, axis, n):
    hinted = check_case(pm, oracle, pw, axis, n, 6, ALL_KINDS, (AMP_G16, AMP_G32), 4)
    # 16 segments (16 lanes) take a hint from 128 positions on, 8 segments (32 lanes, window 11 only) from 64 on
    assert (hinted > 0) == (n >= (64 if pw == 11 else 128)), hinted


@pytest.mark.parametrize("pw, axis", [(11, 0), (11, 1), (5, 0), (5, 1)])
def test_eight_wavefronts_long_chains(pm, oracle, pw, axis):
    assert check_case(pm, oracle, pw, axis, 1690, 6, ALL_KINDS, (AMP_G16, AMP_G32), 8) > 0


@pytest.mark.parametrize("axis", (0, 1))
@pytest.mark.parametrize("n", (31, 32, 33, 63, 64, 65))
def test_two_wavefronts_around_the_shortest_hinted_chain(pm, oracle, axis, n):
    hinted = check_case(pm, oracle, 11, axis, n, 2048, ("head", "runs"), (AMP_G16, AMP_G32), 2)
    assert (hinted > 0) == (n >= 32), hinted       # 4 segments of 32 lanes from 32 positions on, 8 of 16 lanes from 64 on


def test_a_crowd_of_stops_moves_the_boundaries(pm, oracle):
    """that the cases bite: with all predicted stops in the first eighth of a chain the hinted boundaries are NOT the equal
    split, for the run-boundary hint and for the plane"""
    pw, n, chains = 11, 1270, 6
    rows, cols = shape_of(0, pw, n, chains)
    l, r, d = field("head", pw, 0, rows, cols)
    prm = pm.default_params(SEM_CPU, patch=3, patchmatch_iters=1, engine=ENGINE_RUN)
    plane = np.zeros((rows, cols), np.uint8)
    plane[:, :cols // 8] = 1
    with pm.Engine(prm, max_rows=rows, max_cols=cols, max_batch=1) as e:
        for k, mode, st in ((2, RUNS, None), (0, PLANE, plane), (0, RUNS, None)):
            hints = [NONE] * 4
            equal = e.debug_propagate_hinted(l, r, d, pw, pw, 1 << k, AMP_G32, hints, bounds_of=(k, 8))[3]
            hints[k] = mode
            moved = e.debug_propagate_hinted(l, r, d, pw, pw, 1 << k, AMP_G32, hints, stops=st, bounds_of=(k, 8))[3]
            assert equal == pm.segment_bounds(None, n, 8, 32 - pw)
            assert moved != equal and len(moved) == len(equal) == 9, (k, mode, moved)
            # the crowd sits at the left end of the row: in front of a forward sweep, behind a backward one
            crowded, other = (moved[1], equal[1]) if k == 0 else (n - moved[-2], n - equal[-2])
            assert crowded < other, (k, mode, moved)


# ---- Match(): which sweeps are hinted, and that they are ------------------------------------------------------------------
# 64 x 420: row chains of 410 - 416 positions, above the floor of 400 below which no launch takes a hint (the pre-pass does
# not pay on short chains: csrc/pm_seg_bounds.hpp::seg_hint_pays).  The maps cannot show whether a sweep ran hinted -- no
# hint changes a result -- so every case also asserts the host-side decision (pm_debug_match_sweep_hint) and reads the
# stop-bit plane back: it must hold the bits of the LAST iteration that wrote it, which for two iterations is iteration 0,
# whose row +1 sweep the stage hooks reproduce (noise of the iteration's amplitude on the seeds, then the pass).
MATCH_ROWS, MATCH_COLS = 64, 420
MATCH_CASES = [dict(iters=2, windows=(7, 7)), dict(iters=3, windows=(7, 7, 7)), dict(iters=3, windows=(7, 5, 5)),
               dict(iters=3, windows=(11, 11, 7))]


def expected_hints(windows):
    """(mode, write_stops) of the row +1 sweep per iteration: reads where the window is the previous iteration's, writes where
    it is the next one's"""
    n = len(windows)
    return [(PLANE if it > 0 and windows[it - 1] == windows[it] else NONE,
             1 if it + 1 < n and windows[it + 1] == windows[it] else 0) for it in range(n)]


def run_match(pm, oracle, synth, rows, cols, windows):
    p = synth.make_pair(7, rows=rows, cols=cols, n_points=40, dilate_factor=2)
    w = list(windows)
    kw = dict(patchmatch_iters=len(w), patch_w=w, patch_h=w)
    prm = pm.default_params(SEM_CPU, patch=w[-1], **kw)
    with pm.Engine(prm, device=0, max_rows=rows, max_cols=cols) as e:
        dl, dr = e.match(p["left"], p["right"], p["seed_l"], p["seed_r"])
        stops = e.debug_read_stops(0, rows, cols)
        after_first = None
        if len(w) == 2:   # iteration 0's row +1 sweep on its own, from the same seeds and the same unit noise
            noised = e.add_noise(p["seed_l"], float(prm.noise_amp[0]))
            after_first = e.debug_propagate(p["left"], p["right"], noised, w[0], w[0], 1, float(prm.noise_amp[0]))[0]
    el, er = oracle.match(oracle.default_params(SEM_CPU, patch=w[-1], n_iters=len(w), patch_w=w, patch_h=w, nthreads=4),
                          p["left"], p["right"], p["seed_l"], p["seed_r"])
    assert_same(dl, el, f"left {windows} {rows}x{cols}")
    assert_same(dr, er, f"right {windows} {rows}x{cols}")
    return prm, stops, after_first


@pytest.mark.parametrize("case", MATCH_CASES, ids=lambda c: "x".join(map(str, c["windows"])))
def test_match_hands_the_stop_bits_from_one_iteration_to_the_next(pm, oracle, synth, case):
    """Match(): iteration i + 1's row +1 sweep reads the plane iteration i's wrote -- where the window stays; a window that
    changes takes the equal split."""
    rows, cols, w = MATCH_ROWS, MATCH_COLS, case["windows"]
    prm, stops, after_first = run_match(pm, oracle, synth, rows, cols, w)
    want = expected_hints(w)
    for it in range(len(w)):
        assert pm.match_sweep_hint(prm, rows, cols, it, 0) == want[it], (w, it)
        for k in (1, 2, 3):
            assert pm.match_sweep_hint(prm, rows, cols, it, k) == (NONE, 0), (w, it, k)
    assert any(mode == PLANE for mode, _ in want), w          # every case has a hinted sweep
    writer = max(it for it in range(len(w)) if want[it][1])    # the last iteration that stored its bits
    h = w[writer] // 2
    inner = stops[h:rows - h, h:cols - h]
    assert inner.any() and set(np.unique(stops)) <= {0, 1}, w
    outside = stops.copy()
    outside[h:rows - h, h:cols - h] = 0
    if all(x == w[0] for x in w):     # one window: nothing was ever written outside its interior
        assert not outside.any(), w
    if after_first is not None:
        true = (after_first[:, 1:] != after_first[:, :-1]).astype(np.uint8)[h:rows - h, h - 1:cols - h - 1]
        assert np.array_equal(inner, true), (w, int((inner != true).sum()))


@pytest.mark.parametrize("chain_len", (399, 400))
def test_match_chains_below_the_floor_keep_the_equal_split(pm, oracle, synth, chain_len):
    """both sides of kSegHintMinChain: row chains of 399 positions are neither hinted nor do they store stop bits (the plane
    stays as pm_create cleared it), chains of 400 positions are and do"""
    rows, cols, w = 40, chain_len + 6, (7, 7)
    prm, stops, _ = run_match(pm, oracle, synth, rows, cols, w)
    pays = chain_len >= 400
    assert pm.match_sweep_hint(prm, rows, cols, 0, 0) == (NONE, 1 if pays else 0)
    assert pm.match_sweep_hint(prm, rows, cols, 1, 0) == (PLANE if pays else NONE, 0)
    assert bool(stops.any()) == pays
