"""The sweep-kernel variant a launch runs, from the host function that plans it -- no device.

csrc/pm_sweep_plan.hpp::plan_sweep decides engine, lanes per chain segment, wavefronts per chain, compiled-in window and
staged reference lines of every directional sweep; pm_sweeps.hip launches what it returns.  pm_debug_sweep_plan
(include/pm/testing.h) calls it without a handle.  The tables below are DESIGN.md 6, "What selects a sweep kernel variant",
as literals, both sides of every boundary: a retuned threshold fails its rows here, in milliseconds, before
tests/test_sweep_variants.py confirms on the device that what ran is what was planned (and is still right).
"""
import ctypes as C

import numpy as np
import pytest

from test_sweep_variants import chain_geometry

SEM_CPU, SEM_GPU = 0, 1
AUTO, SERIAL, WAVE, RUN = 0, 1, 2, 5     # PM_ENGINE_* (include/pm/patchmatch.h); AUTO runs RUN
PASSES = (0, 1, 2, 3)                    # row +1, column +1, row -1, column -1
NO_NOISE = 1e30


def above(x):
    """the next binary32 above x: what "just above a threshold" is for a float argument"""
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def shape_for(sem, axis, chain_len, chains, window=(3, 3)):
    """(rows, cols) whose sweeps along `axis` have `chains` chains of `chain_len` positions"""
    ph, pw = window
    if sem == SEM_CPU:
        rows, cols = (chains + ph - 1, chain_len + pw - 1) if axis == 0 else (chain_len + ph - 1, chains + pw - 1)
    else:
        rows, cols = (chains + 2, chain_len + 3) if axis == 0 else (chain_len + 3, chains + 2)
    return rows, cols


def plan(pm, sem, window, rows, cols, pass_index, amp=NO_NOISE, slots=1, engine=RUN):
    """-> (engine, group, waves, window, lref) of the planned launch; axis, direction and chain geometry are checked on
    every record."""
    ph, pw = window
    rec = pm.sweep_plan(pm.default_params(sem, engine=engine), rows, cols, ph, pw, pass_index, slots, amp)
    what = (sem, window, rows, cols, pass_index, amp, slots, engine, rec)
    assert (rec["axis"], rec["dir"]) == (pass_index & 1, 1 if pass_index < 2 else -1), what
    assert (rec["chain_len"], rec["chains"]) == chain_geometry(sem, rows, cols, ph, pw, pass_index & 1), what
    return rec["engine"], rec["group"], rec["waves"], rec["window"], rec["lref"]


# ---- window -> kernel, and the group of the windows that have no choice ----------------------------------------------
@pytest.mark.parametrize("window, kernel, group", [((3, 3), 3, 16), ((5, 5), 5, 16), ((7, 7), 7, 32), ((9, 9), 9, 32),
                                                   ((11, 11), 11, 32), ((13, 13), 0, 32), ((3, 7), 0, 32)])
def test_window_selects_the_kernel(pm, window, kernel, group):
    for p in PASSES:   # 43 x 200: short chains, too few for two wavefronts each; row sweeps stage nothing
        assert plan(pm, SEM_CPU, window, 43, 200, p)[:4] == (RUN, group, 4, kernel), (window, p)
    assert plan(pm, SEM_CPU, window, 43, 200, 0, engine=AUTO) == (RUN, group, 4, kernel, 0)


@pytest.mark.parametrize("window, group", [((3, 3), 16), ((5, 5), 16), ((13, 13), 32), ((3, 7), 32), ((7, 3), 32)])
def test_small_windows_take_16_lanes_and_the_general_kernel_32_at_any_amplitude(pm, window, group):
    for p in PASSES:
        for amp in (0.0, 0.25, 0.5, 4.0, 16.0, 32.0, NO_NOISE):
            assert plan(pm, SEM_CPU, window, 43, 200, p, amp)[1] == group, (window, p, amp)


# ---- group of windows 7, 9, 11: 16 lanes up to an amplitude per axis and direction ----------------------------------
@pytest.mark.parametrize("pass_index, threshold", [(0, 0.5), (1, 4.0), (2, 8.0), (3, 16.0)])
@pytest.mark.parametrize("w", [7, 9, 11])
def test_group_threshold_per_axis_and_direction(pm, w, pass_index, threshold):
    at = plan(pm, SEM_CPU, (w, w), 43, 200, pass_index, threshold)
    beyond = plan(pm, SEM_CPU, (w, w), 43, 200, pass_index, above(threshold))
    assert (at[1], beyond[1]) == (16, 32)
    assert at[:1] + at[2:] == beyond[:1] + beyond[2:] == (RUN, 4, w, int(w == 11 and pass_index & 1))
    assert plan(pm, SEM_CPU, (w, w), 43, 200, pass_index, 0.0)[1] == 16
    assert plan(pm, SEM_CPU, (w, w), 43, 200, pass_index, NO_NOISE)[1] == 32


def test_gpu_semantics_take_16_lanes_and_no_window(pm):
    for p in PASSES:
        for amp in (0.0, 0.25, 0.5, 4.0, 8.0, 16.0, 32.0, NO_NOISE):
            for window in ((3, 3), (11, 11)):   # the window is 3 x 3 whatever the caller passes
                rows, cols = 43, 200
                rec = pm.sweep_plan(pm.default_params(SEM_GPU, engine=RUN), rows, cols, *window, p, 1, amp)
                assert (rec["engine"], rec["group"], rec["waves"], rec["window"], rec["lref"]) == (RUN, 16, 4, 0, 0)
                assert (rec["chain_len"], rec["chains"]) == chain_geometry(SEM_GPU, rows, cols, 3, 3, p & 1)


# ---- wavefronts per chain --------------------------------------------------------------------------------------------
#            chain  chains slots waves
WAVE_ROWS = [(1600, 14, 1, 4), (1601, 14, 1, 8),         # 8 beyond 1600 positions
             (399, 2048, 1, 2), (400, 2048, 1, 4),       # 2 below 400 positions ...
             (38, 2047, 1, 4), (38, 2048, 1, 2),         # ... in launches of 2048 chains or more,
             (38, 1024, 1, 4), (38, 1024, 2, 2),         # counted over all slots
             (1, 1, 1, 4), (1, 2048, 64, 2), (1601, 2048, 64, 8)]


@pytest.mark.parametrize("chain_len, chains, slots, waves", WAVE_ROWS)
def test_wavefronts_per_chain(pm, chain_len, chains, slots, waves):
    for p in PASSES:
        for amp, group in ((0.25, 16), (NO_NOISE, 32)):
            rows, cols = shape_for(SEM_CPU, p & 1, chain_len, chains, (11, 11))
            got = plan(pm, SEM_CPU, (11, 11), rows, cols, p, amp, slots)
            assert got[:4] == (RUN, group, waves, 11), (p, amp, got)
        rows, cols = shape_for(SEM_GPU, p & 1, chain_len, chains)
        assert plan(pm, SEM_GPU, (3, 3), rows, cols, p, NO_NOISE, slots) == (RUN, 16, waves, 0, 0), p


# ---- staged reference lines -------------------------------------------------------------------------------------------
def test_window_11_column_sweeps_stage_their_reference_lines_up_to_922_image_rows(pm):
    for p in (1, 3):
        for amp, group in ((0.25, 16), (NO_NOISE, 32)):
            assert plan(pm, SEM_CPU, (11, 11), 922, 30, p, amp) == (RUN, group, 4, 11, 1)
            assert plan(pm, SEM_CPU, (11, 11), 923, 30, p, amp) == (RUN, group, 4, 11, 0)
            assert plan(pm, SEM_CPU, (11, 11), 12, 30, p, amp) == (RUN, group, 4, 11, 1)     # a chain of two positions
            assert plan(pm, SEM_CPU, (11, 11), 922, 4000, p, amp) == (RUN, group, 4, 11, 1)  # the width does not count


def test_nothing_else_stages_reference_lines(pm):
    for p in PASSES:
        for amp in (0.25, NO_NOISE):
            for window in ((3, 3), (5, 5), (7, 7), (9, 9), (13, 13), (3, 7), (11, 5)):
                assert plan(pm, SEM_CPU, window, 43, 60, p, amp)[4] == 0, (window, p)
            assert plan(pm, SEM_GPU, (3, 3), 43, 60, p, amp)[4] == 0
    for p in (0, 2):   # window 11, row sweeps: not even where the row is short
        assert plan(pm, SEM_CPU, (11, 11), 43, 60, p, 0.25) == (RUN, 16, 4, 11, 0)


# ---- engine ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [AUTO, RUN])
def test_chains_beyond_the_lds_fall_back_to_the_serial_engine(pm, engine):
    for axis in (0, 1):
        for p in (axis, axis + 2):
            rows, cols = shape_for(SEM_CPU, axis, 10155, 8, (5, 5))
            assert plan(pm, SEM_CPU, (5, 5), rows, cols, p, engine=engine) == (RUN, 16, 8, 5, 0)
            rows, cols = shape_for(SEM_CPU, axis, 10156, 8, (5, 5))
            assert plan(pm, SEM_CPU, (5, 5), rows, cols, p, engine=engine) == (SERIAL, 0, 0, 0, 0)
            rows, cols = shape_for(SEM_GPU, axis, 8123, 10)
            assert plan(pm, SEM_GPU, (3, 3), rows, cols, p, engine=engine) == (RUN, 16, 8, 0, 0)
            rows, cols = shape_for(SEM_GPU, axis, 8124, 10)
            assert plan(pm, SEM_GPU, (3, 3), rows, cols, p, engine=engine) == (SERIAL, 0, 0, 0, 0)


def test_serial_and_wave_engines_are_reported_as_such(pm):
    for p in PASSES:
        for sem, window in ((SEM_CPU, (11, 11)), (SEM_CPU, (13, 13)), (SEM_GPU, (3, 3))):
            for amp in (0.25, NO_NOISE):
                assert plan(pm, sem, window, 43, 200, p, amp, engine=SERIAL) == (SERIAL, 0, 0, 0, 0)
                assert plan(pm, sem, window, 43, 200, p, amp, engine=WAVE) == (WAVE, 0, 0, 0, 0)
        # PM_SEM_CPU's wave engine keeps no chain in LDS: it stays beyond the limit; PM_SEM_GPU's does, and falls back
        rows, cols = shape_for(SEM_CPU, p & 1, 10156, 8, (5, 5))
        assert plan(pm, SEM_CPU, (5, 5), rows, cols, p, engine=WAVE) == (WAVE, 0, 0, 0, 0)
        rows, cols = shape_for(SEM_GPU, p & 1, 8123, 10)
        assert plan(pm, SEM_GPU, (3, 3), rows, cols, p, engine=WAVE) == (WAVE, 0, 0, 0, 0)
        rows, cols = shape_for(SEM_GPU, p & 1, 8124, 10)
        assert plan(pm, SEM_GPU, (3, 3), rows, cols, p, engine=WAVE) == (SERIAL, 0, 0, 0, 0)


# ---- the hook itself -------------------------------------------------------------------------------------------------
def test_an_empty_interior_gives_an_all_zero_record(pm):
    lib = pm.load()
    prm = pm.default_params(SEM_CPU, engine=RUN)
    for rows, cols in ((6, 200), (43, 6), (7, 7)):   # window 7: no row, no column, one pixel
        for p in PASSES:
            out = pm.PmDebugSweepVariant()
            C.memset(C.byref(out), 0x5a, C.sizeof(out))
            assert lib.pm_debug_sweep_plan(C.byref(prm), rows, cols, 7, 7, p, 1, 1.0, C.byref(out)) == pm.PM_OK
            if (rows, cols) == (7, 7):
                assert (out.engine, out.chain_len, out.chains) == (RUN, 1, 1)
            else:
                assert bytes(out) == bytes(C.sizeof(out)), (rows, cols, p)


def test_invalid_arguments_are_refused(pm):
    lib = pm.load()
    prm = pm.default_params(SEM_CPU, engine=RUN)
    out = pm.PmDebugSweepVariant()
    ok = dict(params=C.byref(prm), pass_index=0, slots=1, amp=1.0, out=C.byref(out))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.pm_debug_sweep_plan(a["params"], 43, 200, 7, 7, a["pass_index"], a["slots"], a["amp"], a["out"])
    assert call() == pm.PM_OK
    bad = [dict(params=None), dict(out=None), dict(pass_index=-1), dict(pass_index=4), dict(slots=0), dict(slots=-3),
           dict(amp=-1.0), dict(amp=-1e-30), dict(amp=float("nan")), dict(amp=float("-inf"))]
    for kw in bad:
        assert call(**kw) == pm.PM_ERR_INVALID_ARG, kw
    assert call(amp=0.0) == pm.PM_OK and call(amp=float("inf")) == pm.PM_OK and call(pass_index=3, slots=64) == pm.PM_OK
    with pytest.raises(pm.PmError) as err:
        pm.sweep_plan(prm, 43, 200, 7, 7, 4)
    assert err.value.status == pm.PM_ERR_INVALID_ARG


# ---- the plan on a host alone, under the sanitizers ------------------------------------------------------------------
def test_the_plan_compiles_without_hip_and_walks_its_grid_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/sweep_plan_main.cpp: csrc/pm_sweep_plan.hpp through g++ (no HIP header in reach) with AddressSanitizer and
    UBSan, over shapes, windows, amplitudes, engines and slot counts, degenerate ones included."""
    import subprocess
    from cpp_build import build_host_kernel
    exe = build_host_kernel(tmp_path / "sweep_plan_main", "sweep_plan_main.cpp", compiler=("g++",),
                            flags=("-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.endswith(" 0 broken\n"), (r.stdout, r.stderr)
