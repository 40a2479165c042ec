"""Where the run engine cuts a chain into segments: csrc/pm_seg_bounds.hpp::segment_bounds, on the host alone.

k_runblk3 cuts every chain into nseg segments that run in parallel.  The boundaries are the equal split, or -- given a
prediction of the positions where the chain's runs stop -- placed at equal cumulative weight, a predicted stop weighing nd
(the positions one run step covers) and any other position 1.  The prediction is a hint: ANY flags must give boundaries
the kernel can run with.  pm_debug_segment_bounds (include/pm/testing.h) exports the function with the kernel's minimum
segment length; tests/test_sweep_segments.py compares what the kernel computes with it on the device.
"""
import numpy as np
import pytest

MIN_LEN = 8                       # csrc/pm_seg_bounds.hpp::kMinSegLen
MAX_SEG, MAX_LEN = 32, 4095       # kSegHintMaxSeg, kSegHintMaxLen: beyond them the equal split
NSEGS = (1, 2, 4, 8, 16, 32)      # (64 / group) * waves for groups 16 / 32 and 1 .. 8 wavefronts
NDS = (1, 5, 6, 21, 22)           # positions per step: 16 / 32 lanes, window 11, row / column sweeps; 1: all weights equal


def equal_split(n, nseg):
    seg_len = max(-(-n // nseg), MIN_LEN)
    return [min(n, s * seg_len) for s in range(nseg)] + [n]


def restated(flags, n, nseg, nd):
    """the rule of the header's comment, written from prefix sums"""
    if flags is None or not np.any(flags) or n < nseg * MIN_LEN or nseg > MAX_SEG or n > MAX_LEN:
        return equal_split(n, nseg)
    w = np.where(np.asarray(flags) != 0, nd, 1).astype(np.int64)
    prefix = np.concatenate(([0], np.cumsum(w)))          # prefix[j] = weight of the first j positions
    total = int(prefix[-1])
    b = [0]
    for s in range(1, nseg):
        target = -(-s * total // nseg)
        j = int(np.searchsorted(prefix, target, side="left"))
        b.append(max(j, b[-1] + MIN_LEN))
    b.append(n)
    for s in range(nseg - 1, 0, -1):
        b[s] = min(b[s], n - (nseg - s) * MIN_LEN)
    return b


def check_invariants(b, n, nseg, hinted, what):
    assert len(b) == nseg + 1 and b[0] == 0 and b[nseg] == n, what
    assert all(0 <= x <= n for x in b), what
    assert all(b[s] <= b[s + 1] for s in range(nseg)), what
    if hinted:   # weighted boundaries: strictly increasing, no segment below the minimum
        assert all(b[s + 1] - b[s] >= MIN_LEN for s in range(nseg)), what


def test_random_flags_keep_the_invariants_and_match_the_restated_rule(pm):
    rng = np.random.default_rng(41)
    for trial in range(400):
        nseg = int(rng.choice(NSEGS))
        nd = int(rng.choice(NDS))
        n = int(rng.integers(1, 40 * nseg + 60)) if trial % 4 else int(rng.integers(1, 2200))
        density = rng.choice([0.0, 0.02, 0.3, 0.9, 1.0])
        flags = (rng.random(n) < density).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)   # any non-zero byte
        b = pm.segment_bounds(flags, n, nseg, nd)
        what = (n, nseg, nd, density)
        check_invariants(b, n, nseg, bool(flags.any()) and n >= nseg * MIN_LEN, what)
        assert b == restated(flags, n, nseg, nd), what


@pytest.mark.parametrize("nseg", NSEGS)
def test_no_hint_is_the_equal_split(pm, nseg):
    for n in (1, 7, 8, nseg * MIN_LEN - 1, nseg * MIN_LEN, nseg * MIN_LEN + 1, 65, 138, 710, 1270, 1700):
        if n < 1:
            continue
        want = equal_split(n, nseg)
        assert pm.segment_bounds(None, n, nseg, 21) == want, n                           # the mode is off
        assert pm.segment_bounds(np.zeros(n, np.uint8), n, nseg, 21) == want, n          # nothing predicted
        check_invariants(want, n, nseg, False, n)


@pytest.mark.parametrize("nseg", NSEGS)
def test_both_sides_of_the_shortest_chain_that_takes_a_hint(pm, nseg):
    rng = np.random.default_rng(nseg)
    for nd in NDS:
        for n in (nseg * MIN_LEN - 1, nseg * MIN_LEN, nseg * MIN_LEN + 1):
            if n < 1:
                continue
            flags = (rng.random(n) < 0.4).astype(np.uint8)
            flags[0] = 1
            b = pm.segment_bounds(flags, n, nseg, nd)
            if n < nseg * MIN_LEN:
                assert b == equal_split(n, nseg), (n, nd)
            else:
                check_invariants(b, n, nseg, True, (n, nd))
                assert b == restated(flags, n, nseg, nd), (n, nd)
                if n == nseg * MIN_LEN:   # no freedom left: every segment is exactly the minimum
                    assert b == [s * MIN_LEN for s in range(nseg + 1)], nd


@pytest.mark.parametrize("nseg", (2, 4, 8, 16, 32))
def test_stops_crowded_at_one_end_are_held_off_by_the_minimum_length(pm, nseg):
    n = 40 * nseg + 3
    for nd in (6, 22):
        first = np.zeros(n, np.uint8)
        first[:MIN_LEN] = 1
        b = pm.segment_bounds(first, n, nseg, nd)
        check_invariants(b, n, nseg, True, ("first", nd))
        assert b == restated(first, n, nseg, nd)
        assert b[1] >= MIN_LEN            # all the weight sits in front of position 8: the minimum acts from the left
        last = np.zeros(n, np.uint8)
        last[n - MIN_LEN:] = 1
        b = pm.segment_bounds(last, n, nseg, nd)
        check_invariants(b, n, nseg, True, ("last", nd))
        assert b == restated(last, n, nseg, nd)
        assert b[nseg - 1] <= n - MIN_LEN  # ... and from the right
    # a crowd heavy enough to pull EVERY boundary into it: the minimum alone spaces them
    n = 64 * nseg
    crowd = np.zeros(n, np.uint8)
    crowd[:4] = 1
    b = pm.segment_bounds(crowd, n, nseg, 100000)
    assert b == [s * MIN_LEN for s in range(nseg)] + [n]
    crowd = np.zeros(n, np.uint8)
    crowd[-4:] = 1
    b = pm.segment_bounds(crowd, n, nseg, 100000)
    assert b == [0] + [n - (nseg - s) * MIN_LEN for s in range(1, nseg)] + [n]


@pytest.mark.parametrize("nseg", NSEGS)
def test_all_flags_set_is_an_even_split_of_the_positions(pm, nseg):
    for n in (nseg * MIN_LEN, 138, 1270, 1700):
        if n < nseg * MIN_LEN:
            continue
        for nd in NDS:
            b = pm.segment_bounds(np.ones(n, np.uint8), n, nseg, nd)
            check_invariants(b, n, nseg, True, (n, nd))
            lens = np.diff(b)
            # equal weights: boundary s at ceil(s n / nseg), unless the minimum moved it
            if n >= nseg * (MIN_LEN + 1):
                assert b == [-(-s * n // nseg) for s in range(nseg)] + [n], (n, nd)
                assert lens.max() - lens.min() <= 1, (n, nd)


def test_beyond_the_kernel_limits_the_equal_split(pm):
    rng = np.random.default_rng(3)
    for n, nseg in ((MAX_LEN + 1, 16), (5000, 32), (1270, 64), (4000, 33)):
        flags = (rng.random(n) < 0.2).astype(np.uint8)
        assert pm.segment_bounds(flags, n, nseg, 21) == equal_split(n, nseg), (n, nseg)
    flags = (rng.random(MAX_LEN) < 0.2).astype(np.uint8)
    b = pm.segment_bounds(flags, MAX_LEN, 32, 21)
    check_invariants(b, MAX_LEN, 32, True, "largest hinted chain")
    assert b == restated(flags, MAX_LEN, 32, 21) and b != equal_split(MAX_LEN, 32)


def test_a_stop_weighs_nd_positions(pm):
    """two segments, one stop: the boundary moves towards the stop's side by about nd / 2 positions"""
    n, nd = 200, 22
    flags = np.zeros(n, np.uint8)
    flags[10] = 1
    b = pm.segment_bounds(flags, n, 2, nd)
    total = n - 1 + nd
    assert b == [0, -(-total // 2) - (nd - 1), n]   # the target lies behind the stop: nd - 1 positions fewer to reach it


def test_refuses_what_it_cannot_index(pm):
    import ctypes as C
    out = (C.c_int * 5)()
    lib = pm.load()
    for n, nseg, nd in ((0, 4, 5), (10, 0, 5), (10, 4, 0), (-1, 4, 5)):
        assert lib.pm_debug_segment_bounds(None, n, nseg, nd, out) == pm.PM_ERR_INVALID_ARG
    assert lib.pm_debug_segment_bounds(None, 10, 4, 5, None) == pm.PM_ERR_INVALID_ARG


# ---- the rule on a host alone, under the sanitizers --------------------------------------------------------------------
def test_the_rule_compiles_without_hip_and_walks_its_grid_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/segment_bounds_main.cpp: csrc/pm_seg_bounds.hpp through g++ (no HIP header in reach) with AddressSanitizer
    and UBSan, flags and boundaries allocated at exactly their sizes, over lengths, segment counts, weights and flag patterns."""
    import subprocess
    from cpp_build import build_host_kernel
    exe = build_host_kernel(tmp_path / "segment_bounds_main", "segment_bounds_main.cpp", compiler=("g++",),
                            flags=("-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.endswith(" 0 broken\n"), (r.stdout, r.stderr)


# ---- which sweeps of a Match() take a hint: the host-side decision -----------------------------------------------------
def test_match_hints_the_row_forward_sweep_of_long_chains_between_iterations_of_one_window(pm):
    """csrc/pm_sweep_plan.hpp::match_sweep_hint through pm_debug_match_sweep_hint: only the row +1 sweep, only chains of at
    least 400 positions (both sides), reading from iteration 1 on where the window is the previous one's, writing where the
    next iteration has the same window."""
    NONE, PLANE = pm.SEG_HINT_NONE, pm.SEG_HINT_PLANE
    floor = pm.SEG_HINT_MIN_CHAIN
    assert floor == 400
    prm = pm.default_params(0, patch=11, patchmatch_iters=4)
    for cols, pays in ((floor - 1 + 10, False), (floor + 10, True), (1280, True), (376, False)):
        got = [pm.match_sweep_hint(prm, 240, cols, it, 0) for it in range(4)]
        want = [(NONE, 1), (PLANE, 1), (PLANE, 1), (PLANE, 0)] if pays else [(NONE, 0)] * 4
        assert got == want, cols
        for it in range(4):
            for k in (1, 2, 3):   # tall images too: the column sweeps' chains being long changes nothing
                assert pm.match_sweep_hint(prm, 1000, cols, it, k) == (NONE, 0), (cols, it, k)
    w = [11, 11, 7, 7, 9]
    prm = pm.default_params(0, patch=9, patchmatch_iters=5, patch_w=w, patch_h=w)
    assert [pm.match_sweep_hint(prm, 100, 600, it, 0) for it in range(5)] == \
        [(NONE, 1), (PLANE, 0), (NONE, 1), (PLANE, 0), (NONE, 0)]
    w, hgt = [7, 7, 7], [7, 9, 9]     # the height counts too
    prm = pm.default_params(0, patch=7, patchmatch_iters=3, patch_w=w, patch_h=hgt)
    assert [pm.match_sweep_hint(prm, 100, 600, it, 0) for it in range(3)] == [(NONE, 0), (NONE, 1), (PLANE, 0)]
    import ctypes as C
    m, wr = C.c_int(), C.c_int()
    lib = pm.load()
    for it, k in ((-1, 0), (3, 0), (0, -1), (0, 4)):
        assert lib.pm_debug_match_sweep_hint(C.byref(prm), 100, 600, it, k, C.byref(m), C.byref(wr)) == pm.PM_ERR_INVALID_ARG
    assert lib.pm_debug_match_sweep_hint(None, 100, 600, 0, 0, C.byref(m), C.byref(wr)) == pm.PM_ERR_INVALID_ARG
