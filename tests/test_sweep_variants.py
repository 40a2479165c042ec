"""Every kernel variant of the directional sweeps, one sweep at a time, on crafted fields, against the oracle.

plan_sweep (csrc/pm_sweep_plan.hpp) picks one of several dozen instantiations of k_runblk3 / k_runblk2 per launch -- by
the window, the iteration's noise amplitude, the chain length, the chain count and the image height -- and launch_sweep
(csrc/pm_sweeps.hip) launches it; pm_propagate, with its fixed "no noise" amplitude and its small images, meets about one
in six of them.  pm_debug_propagate (include/pm/testing.h) takes the amplitude as an argument and reports the variant
every pass ran.  Each case below

  * compares the map after the sweep(s) with oracle.cpu_propagate / oracle.gpu_propagate at tolerance 0,
  * asserts that the record of what ran equals what pm_debug_sweep_plan plans for the same parameters, shape, pass and
    amplitude without a device (tests/test_sweep_plan.py pins that plan on the CPU), and
  * asserts the variant record it was written for: a case that means to cover 16-lane groups, two wavefronts per chain or
    staged reference lines FAILS when a retuned threshold makes it cover something else.  The remedy is then another
    amplitude or shape in the case, never a weaker comparison.

The fields are those of the stage tests of tests/test_gpu_parity.py (tests/sweep_fields.py): lerp weights of 0 and 65536,
one value that runs through every chain segment, and PM_SEM_GPU's clamp / plateau / binade fields.  The last test asserts
that the cases together have shown every variant; a case that has not run yet (a -k selection) is run by it.
Wavefronts per chain are asserted on EVERY run-engine record, against plan_sweep's rule restated here (runblk_waves) and,
on the axis a case is about, against the count the case was written for.
"""
import functools

import numpy as np
import pytest

import sweep_fields
from conftest import assert_same

pytestmark = pytest.mark.gpu

SEM_CPU, SEM_GPU = 0, 1
ENGINE_SERIAL, ENGINE_RUN = 1, 5        # PM_ENGINE_SERIAL, PM_ENGINE_RUNBLK2 (include/pm/patchmatch.h)
ALL_MASKS = (1, 2, 4, 8, 15)            # bit k: 0 = row +1, 1 = column +1, 2 = row -1, 3 = column -1
AXIS_MASKS = {0: (1, 4, 5), 1: (2, 8, 10)}
# Noise amplitudes: plan_sweep takes 16-lane groups for windows 7 / 9 / 11 where the amplitude is at most a threshold per
# axis and direction (the smallest is the forward row sweeps'); 0.25 lies under all four, 1e30 -- pm_propagate's -- above.
AMP_G16, AMP_G32 = 0.25, 1e30

# ---- the host-side formulas the shapes below are derived from, restated (the records confirm them) --------------------
K_WAVE, K_MAX_SEG_WAVES = 64, 16                   # csrc/pm_sweep_defs.hpp
K_CHAIN_LDS_MAX = 160 * 1024 - 1024                # csrc/pm_sweep_defs.hpp
K_LREF4_STRIDE, LREF_LIMIT = 7, 40 * 1024          # csrc/pm_sweep_defs.hpp, pm_sweep_plan.hpp::SweepKnobs::lref_limit


def chain_lds_bytes(n, planes):
    """chain_lds_bytes(n, 4 * kMaxSegWaves + 4, planes) of plan_sweep: beyond K_CHAIN_LDS_MAX the serial engine runs."""
    return 4 * (planes * ((n + 1 + 3) & ~3) + 4 * K_MAX_SEG_WAVES + 4)


def longest_chain_in_lds(sem):
    planes = 4 if sem == SEM_CPU else 5
    n = 1
    while chain_lds_bytes(n + 1, planes) <= K_CHAIN_LDS_MAX:
        n += 1
    return n


def lref_stages(rows, ph=11):
    """plan_sweep, window 11: column sweeps stage their reference lines while the chain state (sized for 64
    segments) and kLref4Stride dwords per image row fit the budget."""
    n = rows - (ph - 1)
    return 4 * (4 * (n + 1) + 2 * 64 + 3) + 4 * K_LREF4_STRIDE * rows <= LREF_LIMIT


def tallest_staged_image():
    rows = 12
    while lref_stages(rows + 1):
        rows += 1
    return rows


def runblk_waves(chain_len, chains):
    """plan_sweep's rule for one slot: wavefronts per chain"""
    return 8 if chain_len > 1600 else 2 if (chain_len < 400 and chains >= 2048) else 4


def chain_geometry(sem, rows, cols, ph, pw, axis):
    """(chain length, chains) of a sweep along `axis`: the interior of csrc/pm_engine.hip::interior / sweep_geom"""
    if sem == SEM_CPU:
        along, across = (cols - (pw - 1), rows - (ph - 1))
        return (along, across) if axis == 0 else (across, along)
    return (cols - 3, rows - 2) if axis == 0 else (rows - 3, cols - 2)


# ---- fields, oracle results, the runner --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def make_field(synth, key):
    kind = key[0]
    if kind == "weights":
        return sweep_fields.weight_extremes(synth, *key[1:])            # (pw, rows, cols)
    if kind == "runs":
        return sweep_fields.one_value_runs(*key[1:])                    # (pw, layout, rows, cols)
    return sweep_fields.gpu_adversarial(synth, *key)                    # (kind, rows, cols)


SEEN = set()        # (semantics, engine, axis, group, waves, window, lref) of every record of every case
LIMIT_SEEN = set()  # (semantics, engine) either side of the LDS limit (section d)


def run_sweeps(pm, oracle, synth, sem, ph, pw, key, amps, masks, expect, after_pass=None, counters=False):
    """Runs every mask at every amplitude on the field `key`, compares with the oracle, checks every record's geometry and
    calls expect(record, amp) on it.  after_pass(engine, mask, want): extra assertions on one pass."""
    l, r, d = make_field(synth, key)
    rows, cols = d.shape
    ims = oracle.ImageSet(l, r)
    prm = pm.default_params(sem, patch=3, patchmatch_iters=1, engine=ENGINE_RUN)
    out = {}
    with pm.Engine(prm, max_rows=rows, max_cols=cols, max_batch=1) as e:
        if counters:
            e.debug_counters_enable()
        for mask in masks:
            if sem == SEM_CPU:
                want = oracle.cpu_propagate(ims, d, ph, pw, pass_mask=mask, nthreads=8)
            else:
                want = oracle.gpu_propagate(ims, d, pass_mask=mask, nthreads=8)
            for amp in amps:
                if counters:
                    e.debug_counters()   # reading resets them
                got, recs = e.debug_propagate(l, r, d, ph, pw, mask, amp)
                what = f"{key} window {ph}x{pw} pass mask {mask} amp {amp}"
                assert_same(got, want, what)
                passes = [k for k in range(4) if mask & (1 << k)]
                assert len(recs) == len(passes), what
                for k, rec in zip(passes, recs):
                    assert (rec["axis"], rec["dir"]) == (k & 1, 1 if k < 2 else -1), (what, rec)
                    assert (rec["chain_len"], rec["chains"]) == chain_geometry(sem, rows, cols, ph, pw, k & 1), (what, rec)
                    # what ran is what was planned
                    assert rec == pm.sweep_plan(prm, rows, cols, ph, pw, k, 1, amp), (what, rec)
                    expect(rec, amp, what)
                    SEEN.add((sem, rec["engine"], rec["axis"], rec["group"], rec["waves"], rec["window"], rec["lref"]))
                out[mask, amp] = recs
                if after_pass:
                    after_pass(e, mask, want, what)
    return out


def once(fn):
    """A case runs once per session, pass or fail: the coverage test at the end of the file calls every case, so that it
    holds under a -k selection too, and must neither repeat the work nor report a failed case a second time."""
    done = set()

    @functools.wraps(fn)
    def wrapper(pm, oracle, synth, *args):
        if args not in done:
            done.add(args)
            fn(pm, oracle, synth, *args)
    return wrapper


def case_id(case):
    return "-".join("x".join(map(str, a)) if isinstance(a, tuple) else str(a) for a in case)


def fixed_window(ph, pw):
    return pw if (ph == pw and pw <= 11) else 0       # plan_sweep: the compiled-in windows


def expect_waves(rec, waves, what):
    """Every run-engine record carries the wavefronts per chain runblk_waves() gives its chain length and chain count;
    waves = {axis: wavefronts}: what the case was written for on that axis -- a retuned bucket fails the case."""
    assert rec["waves"] == runblk_waves(rec["chain_len"], rec["chains"]), (what, rec)
    if rec["axis"] in waves:
        assert rec["waves"] == waves[rec["axis"]], (what, rec)


def expect_cpu_run(ph, pw, rows, waves):
    """The record of a PM_SEM_CPU run-engine launch: the window's kernel, the amplitude's group where the window has a
    choice, staged reference lines exactly for window 11 / column sweeps / images that fit, the wavefronts per chain."""
    tp = fixed_window(ph, pw)

    def expect(rec, amp, what):
        assert rec["engine"] == ENGINE_RUN and rec["window"] == tp, (what, rec)
        group = 16 if tp in (3, 5) else 32 if tp == 0 else (16 if amp == AMP_G16 else 32)
        assert rec["group"] == group, (what, rec)
        assert rec["lref"] == int(tp == 11 and rec["axis"] == 1 and lref_stages(rows)), (what, rec)
        expect_waves(rec, waves, what)
    return expect


def expect_gpu_run(waves):
    def expect(rec, amp, what):   # PM_SEM_GPU: k_runblk2 with 16-lane groups whatever the amplitude
        assert (rec["engine"], rec["group"], rec["window"], rec["lref"]) == (ENGINE_RUN, 16, 0, 0), (what, rec)
        expect_waves(rec, waves, what)
    return expect


# ---- a. lanes per segment x window x pass --------------------------------------------------------------------------------
# 43 rows: column chains of 33 positions in which most of the 8 / 16 segments are empty (a segment is at least 8 positions
# long), and rows % 8 != 0 for the leftover loop of the reference-line staging; 48 rows: no leftover.  22 x 900 and 900 x 52:
# chains of 890 positions, 8 / 16 segments, the value handed over between them in the fix-up rounds.  All of that holds at
# FOUR wavefronts per chain (64 / GS segments per wavefront), which every record of this section is asserted to have.
A_WINDOWS = [(7, 7), (9, 9), (11, 11), (3, 3), (5, 5), (13, 13), (3, 7)]      # (patch_height, patch_width)
A_FIELDS = [("weights", 43, 200), ("weights", 48, 200), ("runs", "rows", 22, 900), ("runs", "cols", 900, 52)]
A_CASES = [(w, f) for w in A_WINDOWS for f in A_FIELDS]


@once
def check_group_window_pass(pm, oracle, synth, window, field):
    ph, pw = window
    key = (field[0], pw) + field[1:]
    rows = field[-2]
    after = None
    if field[0] == "runs":
        long_mask, axis_name = (1, "row") if field[1] == "rows" else (2, "col")

        def after(e, mask, want, what):
            if mask == long_mask:
                assert (want == sweep_fields.RUN_VALUE).mean() > 0.2, what        # the value did run far
                c = e.debug_counters()[axis_name]
                assert c["fixup_rounds"] > 0 and c["steps_fixup"] > 0, (what, c)  # ... and was handed over
    got = run_sweeps(pm, oracle, synth, SEM_CPU, ph, pw, key, (AMP_G16, AMP_G32), ALL_MASKS,
                     expect_cpu_run(ph, pw, rows, {0: 4, 1: 4}), after, counters=after is not None)
    if fixed_window(ph, pw) not in (7, 9, 11):   # no choice of group: the amplitude changes nothing in the record
        for mask in ALL_MASKS:
            assert got[mask, AMP_G16] == got[mask, AMP_G32], (window, field, mask)


@pytest.mark.parametrize("case", A_CASES, ids=case_id)
def test_group_window_pass(pm, oracle, synth, case):
    check_group_window_pass(pm, oracle, synth, *case)


# ---- b. wavefronts per chain: the smallest shapes of each bucket, and both sides of each boundary ----------------------
# runblk_waves(): 8 for chains longer than 1600, 2 for chains shorter than 400 in launches of at least 2048 chains, else 4.
# (shape, the axis the shape is about, wavefronts per chain there); 4 is what the short axis of the first two takes
B_SHAPES = [((24, 1700), 0, 8), ((1700, 40), 1, 8), ((2100, 48), 0, 2), ((40, 2100), 1, 2)]
B_CPU_CASES = [(pw, s) for pw in (11, 5) for s in B_SHAPES]
B_GPU_CASES = [(kind, s) for kind in sweep_fields.GPU_ADVERSARIAL_KINDS for s in B_SHAPES]


@once
def check_wave_bucket_cpu(pm, oracle, synth, pw, bucket):
    (rows, cols), axis, waves = bucket
    key = ("runs", pw, "rows" if axis == 0 else "cols", rows, cols)
    run_sweeps(pm, oracle, synth, SEM_CPU, pw, pw, key, (AMP_G16, AMP_G32), ALL_MASKS,
               expect_cpu_run(pw, pw, rows, {axis: waves}))


@once
def check_wave_bucket_gpu(pm, oracle, synth, kind, bucket):
    (rows, cols), axis, waves = bucket
    run_sweeps(pm, oracle, synth, SEM_GPU, 3, 3, (kind, rows, cols), (AMP_G16, AMP_G32), ALL_MASKS,
               expect_gpu_run({axis: waves}))


@pytest.mark.parametrize("case", B_CPU_CASES, ids=case_id)
def test_wave_bucket_cpu_semantics(pm, oracle, synth, case):
    check_wave_bucket_cpu(pm, oracle, synth, *case)


def test_window_11_column_sweeps_of_a_tall_image_read_their_reference_from_memory(pm, oracle, synth):
    """1700 x 40 is also the LREF = false case of the window-11 column sweeps, 40 x 2100 the staged one."""
    assert not lref_stages(1700) and lref_stages(40)
    check_wave_bucket_cpu(pm, oracle, synth, 11, B_SHAPES[1])   # expect_cpu_run asserts the record against lref_stages
    check_wave_bucket_cpu(pm, oracle, synth, 11, B_SHAPES[3])
    for lref in (0, 1):
        for group in (16, 32):
            assert {w for (s, e, a, g, w, tp, lr) in SEEN if (s, a, g, tp, lr) == (SEM_CPU, 1, group, 11, lref)}, (lref, group)


@pytest.mark.parametrize("case", B_GPU_CASES, ids=case_id)
def test_wave_bucket_gpu_semantics(pm, oracle, synth, case):
    check_wave_bucket_gpu(pm, oracle, synth, *case)


# (what varies, axis, window, chain length, chains, amplitudes, pass masks, wavefronts per chain): pairs either side of a
# boundary, one position or one chain apart.  Chains shorter than 400 take two wavefronts only in launches of 2048 chains or
# more, so the 399 / 400 pair has that many chains -- 800 000 positions, swept by the two single passes only.  On the
# column axis that pair is also the longest staged-reference (LREF) chains of the file: 409 image rows, window 11.
B_BOUNDARY_CASES = []
for _axis in (0, 1):
    _both, _single = AXIS_MASKS[_axis], AXIS_MASKS[_axis][:2]
    B_BOUNDARY_CASES += [("len", _axis, 11, 1600, 14 + 16 * _axis, (AMP_G16, AMP_G32), _both, 4),
                         ("len", _axis, 11, 1601, 14 + 16 * _axis, (AMP_G16, AMP_G32), _both, 8),
                         ("len", _axis, 11, 399, 2048, (AMP_G16, AMP_G32), _single, 2),
                         ("len", _axis, 11, 400, 2048, (AMP_G16, AMP_G32), _single, 4),
                         ("chains", _axis, 11, 38, 2047, (AMP_G16,), _both, 4),
                         ("chains", _axis, 11, 38, 2048, (AMP_G16,), _both, 2)]


@once
def check_wave_boundary(pm, oracle, synth, what, axis, pw, chain_len, chains, amps, masks, waves):
    along, across = chain_len + pw - 1, chains + pw - 1
    rows, cols = (across, along) if axis == 0 else (along, across)
    key = ("runs", pw, "rows" if axis == 0 else "cols", rows, cols)
    got = run_sweeps(pm, oracle, synth, SEM_CPU, pw, pw, key, amps, masks,
                     expect_cpu_run(pw, pw, rows, {axis: waves}))
    for recs in got.values():   # the shape is what the case says it is
        assert all((rec["chain_len"], rec["chains"]) == (chain_len, chains) for rec in recs), recs


@pytest.mark.parametrize("case", B_BOUNDARY_CASES, ids=case_id)
def test_wave_bucket_boundaries(pm, oracle, synth, case):
    check_wave_boundary(pm, oracle, synth, *case)


# ---- c. the tallest image whose window-11 column sweeps stage their reference lines, and one row more -------------------
C_CASES = [0, 1]   # rows beyond tallest_staged_image()


@once
def check_lref_limit(pm, oracle, synth, beyond):
    rows = tallest_staged_image() + beyond
    assert lref_stages(rows) == (beyond == 0)
    got = run_sweeps(pm, oracle, synth, SEM_CPU, 11, 11, ("runs", 11, "cols", rows, 30), (AMP_G16, AMP_G32), (2, 8),
                     expect_cpu_run(11, 11, rows, {1: 4}))
    assert all(rec["lref"] == 1 - beyond for recs in got.values() for rec in recs), got


@pytest.mark.parametrize("beyond", C_CASES)
def test_lref_limit(pm, oracle, synth, beyond):
    check_lref_limit(pm, oracle, synth, beyond)


# ---- d. the longest chain the run engines hold in LDS, and one position more (the serial engine) -----------------------
D_CASES = [(SEM_CPU, "runs", b) for b in (0, 1)] + [(SEM_GPU, k, b) for k in sweep_fields.GPU_ADVERSARIAL_KINDS for b in (0, 1)]


@once
def check_lds_limit(pm, oracle, synth, sem, field, beyond):
    n = longest_chain_in_lds(sem) + beyond
    engine = ENGINE_SERIAL if beyond else ENGINE_RUN
    rows = 12
    if sem == SEM_CPU:
        pw, key = 5, ("runs", 5, "rows", rows, n + 4)
        run_expect = expect_cpu_run(5, 5, rows, {0: 8})   # 16 segments of about 635 positions
    else:
        pw, key = 3, (field, rows, n + 3)
        run_expect = expect_gpu_run({0: 8})

    def expect(rec, amp, what):
        assert (rec["engine"], rec["chain_len"]) == (engine, n), (what, rec)
        if beyond:
            assert (rec["group"], rec["waves"], rec["window"], rec["lref"]) == (0, 0, 0, 0), (what, rec)
        else:
            run_expect(rec, amp, what)
        LIMIT_SEEN.add((sem, rec["engine"]))
    run_sweeps(pm, oracle, synth, sem, pw, pw, key, (AMP_G16, AMP_G32), AXIS_MASKS[0], expect)


@pytest.mark.parametrize("case", D_CASES, ids=case_id)
def test_lds_limit(pm, oracle, synth, case):
    check_lds_limit(pm, oracle, synth, *case)


# ---- the hook itself --------------------------------------------------------------------------------------------------
def test_hook_is_pm_propagate_and_refuses_amplitudes_that_are_not_at_least_zero(pm, synth):
    l, r, d = sweep_fields.weight_extremes(synth, 7, 43, 200)
    with pm.Engine(pm.default_params(SEM_CPU, patch=3, patchmatch_iters=1, engine=ENGINE_RUN), max_rows=43, max_cols=200,
                   max_batch=1) as e:
        got, recs = e.debug_propagate(l, r, d, 7, 7, 10)          # the default amplitude is pm_propagate's
        assert_same(got, e.propagate(l, r, d, 7, 7, 10), "pm_debug_propagate vs pm_propagate")
        assert [(rec["axis"], rec["dir"], rec["group"]) for rec in recs] == [(1, 1, 32), (1, -1, 32)]
        for amp in (-1.0, -1e-30, float("nan"), float("-inf")):
            with pytest.raises(pm.PmError) as err:
                e.debug_propagate(l, r, d, 7, 7, 15, amp)
            assert err.value.status == pm.PM_ERR_INVALID_ARG and "pm_debug_propagate" in str(err.value), amp
            assert "amplitude" in str(err.value), amp
        # a refused call leaves no stale record behind, and names the entry point that was called
        import ctypes as C
        l, r = np.ascontiguousarray(l, np.uint8), np.ascontiguousarray(r, np.uint8)
        ran = (pm.PmDebugSweepVariant * 4)()
        C.memset(ran, 0x5a, C.sizeof(ran))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        assert e.lib.pm_debug_propagate(e.h, ptr(l), ptr(r), 43, 200, ptr(d.copy()), 7, 7, 15, -1.0, ran) == pm.PM_ERR_INVALID_ARG
        assert bytes(ran) == bytes(C.sizeof(ran))
        bad = d.copy()
        bad[20, 100] = -1.0
        C.memset(ran, 0x5a, C.sizeof(ran))
        assert e.lib.pm_debug_propagate(e.h, ptr(l), ptr(r), 43, 200, ptr(bad), 7, 7, 15, 1.0, ran) == pm.PM_ERR_INVALID_ARG
        assert bytes(ran) == bytes(C.sizeof(ran)) and b"pm_debug_propagate" in e.lib.pm_last_error(e.h)
        with pytest.raises(pm.PmError, match="pm_propagate"):
            e.propagate(l, r, bad, 7, 7, 15)
        assert e.debug_propagate(l, r, d, 7, 7, 1, 0.0)[1][0]["group"] == 16   # zero is an amplitude


# ---- the cases together show every variant ------------------------------------------------------------------------------
def test_the_cases_cover_every_variant(pm, oracle, synth):
    for check, cases in ((check_group_window_pass, A_CASES), (check_wave_bucket_cpu, B_CPU_CASES),
                         (check_wave_bucket_gpu, B_GPU_CASES), (check_wave_boundary, B_BOUNDARY_CASES),
                         (check_lref_limit, [(b,) for b in C_CASES]), (check_lds_limit, D_CASES)):
        for case in cases:
            check(pm, oracle, synth, *case)   # returns at once where the case has run
    run = [v for v in SEEN if v[1] == ENGINE_RUN]
    cpu = [v for v in run if v[0] == SEM_CPU]
    # every window kernel with every group it admits, in both directions of both axes (the passes of mask 15)
    windows = {(tp, g) for (_, _, _, g, _, tp, _) in cpu}
    assert windows == {(3, 16), (5, 16), (7, 16), (7, 32), (9, 16), (9, 32), (11, 16), (11, 32), (0, 32)}, windows
    for axis in (0, 1):
        assert {(tp, g) for (_, _, a, g, _, tp, _) in cpu if a == axis} == windows, axis
    # 2, 4 and 8 wavefronts per chain on both axes for both semantics
    for sem in (SEM_CPU, SEM_GPU):
        for axis in (0, 1):
            assert {w for (s, _, a, _, w, _, _) in run if (s, a) == (sem, axis)} == {2, 4, 8}, (sem, axis)
    assert {g for (s, _, _, g, _, _, _) in run if s == SEM_GPU} == {16}
    # window 11, column sweeps: reference lines staged and not, with both groups; nothing else stages
    assert {(g, lr) for (_, _, a, g, _, tp, lr) in cpu if (a, tp) == (1, 11)} == {(16, 0), (16, 1), (32, 0), (32, 1)}
    assert all((a, tp) == (1, 11) for (_, _, a, _, _, tp, lr) in run if lr)
    # both engines either side of the LDS limit
    assert LIMIT_SEEN == {(sem, eng) for sem in (SEM_CPU, SEM_GPU) for eng in (ENGINE_RUN, ENGINE_SERIAL)}, LIMIT_SEEN
