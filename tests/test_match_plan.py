"""The route of a Match() call, from the host function that plans it -- no device.

csrc/pm_match_plan.hpp::plan_match decides which launches of a call go onto which stream: the route, which views seed
themselves on the device, pairs per chunk and whether a chunk's head runs aside, plane mode's lanes, how the frames of a
sequence run, and what must exist before a capture opens.  pm_debug_match_plan (include/pm/testing.h) calls it without a
handle.  The tables below are DESIGN.md 6, "The routes of a Match()", as literals, both sides of every boundary;
tests/test_match_schedule.py counts on the device what each route launches.
"""
import ctypes as C
import itertools

import pytest

PLANES, ONE_STREAM, SHARED_HEAD, VIEW_HEADS, CHUNKS = 0, 1, 2, 3, 4   # pm_debug_match_route.route


def params(pm, lr=1, planes=False, **kw):
    if planes:
        kw.update(mode=pm.PM_MODE_PLANES, max_disp=48)
    return pm.default_params(0, patch=7, left_right_check=lr, **kw)


# ---- the route: the "when" column ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr, bgr, n, route", [
    (1, False, 1, VIEW_HEADS), (1, False, 2, VIEW_HEADS), (1, False, 3, CHUNKS),   # gray, two views: chunks from n = 3 on
    (0, False, 1, ONE_STREAM), (0, False, 3, ONE_STREAM), (0, False, 32, ONE_STREAM),   # one view: any n
    (1, True, 1, SHARED_HEAD), (1, True, 3, SHARED_HEAD),                          # BGR input, two views: any n
    (0, True, 1, ONE_STREAM), (0, True, 3, ONE_STREAM)])
def test_scalar_routes(pm, lr, bgr, n, route):
    for seeded in (False, True):
        rec = pm.match_plan(params(pm, lr), n, seeded, seeded, bgr)
        assert (rec["route"], rec["n_views"], rec["pair_chunk"]) == (route, 2 if lr else 1, 2), (lr, bgr, n, rec)
        assert rec["lane_pairs"] == (0, 0)
    assert pm.ROUTE_CHUNKS == CHUNKS and pm.ROUTE_PLANES == PLANES


@pytest.mark.parametrize("n, lanes", [(1, (1, 0)), (2, (1, 1)), (3, (2, 1)), (4, (2, 2)), (5, (3, 2))])
def test_plane_mode_lanes(pm, n, lanes):
    for lr, bgr in itertools.product((0, 1), (False, True)):
        rec = pm.match_plan(params(pm, lr, planes=True), n, True, True, bgr)
        assert (rec["route"], rec["lane_pairs"], rec["n_views"]) == (PLANES, lanes, 2 if lr else 1), (n, lr, bgr, rec)


# ---- which views seed themselves, and whether a chunk's head runs aside ----------------------------------------------
@pytest.mark.parametrize("sparse, given_l, given_r, lr", list(itertools.product((0, 1), (False, True), (False, True), (0, 1))))
def test_self_seeding_and_head_aside(pm, sparse, given_l, given_r, lr):
    s0 = 1 if sparse and not given_l else 0
    s1 = 1 if sparse and not given_r and lr else 0            # the second view exists with left_right_check only
    for planes, n in itertools.product((False, True), (1, 3)):
        rec = pm.match_plan(params(pm, lr, planes=planes, sparse_init=sparse), n, given_l, given_r)
        what = (sparse, given_l, given_r, lr, planes, n, rec)
        assert rec["self_seed"] == (s0, s1), what
        assert rec["head_aside"] == (1 if s0 + s1 > 0 else 0), what   # exactly when a view seeds itself


# ---- frame sequences -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr, planes, chunks, hold", [(1, False, 1, 1), (0, False, 0, 0), (1, True, 0, 1), (0, True, 0, 1)])
def test_sequences(pm, lr, planes, chunks, hold):
    for sparse, n in itertools.product((0, 1), (1, 2, 5)):
        rec = pm.match_plan(params(pm, lr, planes=planes, sparse_init=sparse), n)
        assert (rec["seq_chunks"], rec["seq_hold"]) == (chunks, hold), (lr, planes, sparse, n, rec)


# ---- what a capture needs ahead of it --------------------------------------------------------------------------------
@pytest.mark.parametrize("lr, planes, sparse", list(itertools.product((0, 1), (False, True), (0, 1))))
def test_pre_capture_needs(pm, lr, planes, sparse):
    rec = pm.match_plan(params(pm, lr, planes=planes, sparse_init=sparse), 1)
    events = 1 if lr and not planes else 0   # the fork / join events of the views and the per-slot events of chunks
    assert (rec["need_view_events"], rec["need_slot_events"], rec["need_second_seed_scratch"]) == (events, events, sparse), rec


# ---- the hook itself -------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused(pm):
    lib = pm.load()
    pm.match_plan(params(pm), 1)   # (sets the argument types)
    prm, out = params(pm), pm.PmDebugMatchRoute()
    assert lib.pm_debug_match_plan(C.byref(prm), 1, 0, 0, 0, C.byref(out)) == pm.PM_OK
    assert lib.pm_debug_match_plan(None, 1, 0, 0, 0, C.byref(out)) == pm.PM_ERR_INVALID_ARG
    assert lib.pm_debug_match_plan(C.byref(prm), 1, 0, 0, 0, None) == pm.PM_ERR_INVALID_ARG
    for n in (0, -1):
        assert lib.pm_debug_match_plan(C.byref(prm), n, 0, 0, 0, C.byref(out)) == pm.PM_ERR_INVALID_ARG
    with pytest.raises(pm.PmError) as err:
        pm.match_plan(prm, 0)
    assert err.value.status == pm.PM_ERR_INVALID_ARG


# ---- the plan on a host alone, under the sanitizers ------------------------------------------------------------------
def test_the_plan_compiles_without_hip_and_walks_its_grid_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/match_plan_main.cpp: csrc/pm_match_plan.hpp through g++ (no HIP header in reach) with AddressSanitizer and
    UBSan, over modes, view counts, batch sizes, seed maps, input kinds and knobs."""
    import subprocess
    from cpp_build import build_host_kernel
    exe = build_host_kernel(tmp_path / "match_plan_main", "match_plan_main.cpp", compiler=("g++",),
                            flags=("-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.endswith(" 0 broken\n"), (r.stdout, r.stderr)
