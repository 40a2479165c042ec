"""PM_MODE_PLANES stage by stage, at tile, parity and image edges, on crafted states, against the definition.

One kernel template (csrc/pm_planes.hpp::k_planes) runs every stage of the mode, instantiated 5 stages x 7 windows x 2 state
types x 2 window shapes; which instantiation a launch takes, its grid, its LDS and the way it fills its target tile follow
from the parameters and the image size in ONE host function (csrc/pm_planes_plan.hpp::plan_planes), which the launch is made
from.  pm_debug_planes_plan (include/pm/testing.h) returns that plan without a device, pm_debug_planes_last the record of
what a handle's last stage launched.  Every GPU case below

  * compares all four planes (a, b, z, cost) of every view after EVERY stage with oracle.PlanesViews at tolerance 0 -- bit
    identity with oracle/pm_planes_oracle.c is this mode's contract, and a one-candidate defect that three iterations of a
    whole Match() heal cannot hide behind a single stage,
  * asserts that the record of what ran equals pm_debug_planes_plan for the same arguments, and
  * asserts the variant it was written for: a case that means to cover a partial tile, the fast fill or the register
    window FAILS when a retuned constant makes it cover something else.  The remedy is then another shape in the case,
    never a weaker comparison.

Shapes come from pm_debug_planes_constants, not from literals.  The CPU part pins the plan against its restatement here
and shows, with the definition's arithmetic alone, that every crafted field (tests/plane_fields.py) reaches the branch it
is named for.  The last test asserts that the records seen cover every (stage, window, window shape, state type, fill
path); a case a -k selection skipped is run by it.

Sizes: every entry point of the library takes images of 8 x 8 and more (include/pm/patchmatch.h), plane mode included;
smaller ones -- and the 7-row shapes below a tile edge -- are REFUSED by that rule, by pm_planes_begin, by Match() and by
the definition's Python wrapper alike, and the refusal is what is tested for them (test_images_below_the_rule_are_refused).
"""
import functools
import itertools
import math

import numpy as np
import pytest

import plane_fields as F
from conftest import assert_same

gpu = pytest.mark.gpu

INIT, SPATIAL, VIEW, REFINE, VIEW_REFINE = 0, 1, 2, 3, 4      # stage ids: 0 = pm_planes_begin's launch, else PM_PL_*
STAGES = (INIT, SPATIAL, VIEW, REFINE, VIEW_REFINE)
WIDE_STAGES = (INIT, VIEW, REFINE, VIEW_REFINE)                  # one pixel per lane; SPATIAL: one colour of a wider tile
WINDOWS = (3, 5, 7, 9, 11, 13, 15)
CHECKER, FULL = 1, 0
FOUR, TWO = 0, 1
MIN_SIZE = 8                                                     # the library's rule for rows and cols
K_CHAIN_LDS_MAX = 160 * 1024 - 1024                              # csrc/pm_sweep_defs.hpp
NAMES = "a b z cost".split()


# ---- parameters, and plan_planes restated --------------------------------------------------------------------------------
def pparams(pm, patch=11, iters=2, f16=0, **kw):
    kw.setdefault("state_dtype", f16)
    kw.setdefault("mode", pm.PM_MODE_PLANES)
    return pm.default_params(0, patch=patch, patchmatch_iters=iters, **kw)


def oparams(oracle, prm):
    return oracle.planes_params(**oracle.planes_kwargs_of(prm, nthreads=4))


def pair_order(P):
    """PlPairOrder<P> (csrc/pm_planes_plan.hpp): taps of an even / odd checkerboard row, whole groups of four, leftovers."""
    NE, NO = (P + 1) // 2, P // 2
    QE, QO, RE, RO = NE // 4, NO // 4, NE % 4, NO % 4
    return dict(NE=NE, NO=NO, QE=QE, QO=QO, RE=RE, RO=RO, shared=RE > 0 and RO > 0 and RE + RO <= 4)


def tap_class(P, window):
    o = pair_order(P)
    return 4 * o["RE"] + o["RO"] if window == CHECKER else 16 + P % 4


def ref_row_dwords(LW, window):
    return ((LW + 1) // 2 + 3) // 4 + 1 if window == CHECKER else (LW + 3) // 4 + 1


def slope_margin(prm):
    smax = float(np.float32(prm.plane_slope_max))
    if prm.state_dtype == 1:
        smax = float(np.float16(smax))
    return int(math.ceil(2.0 * (prm.patch_w[0] // 2) * smax)) + 2


def expected_plan(pm, prm, stage, rows, cols):
    """plan_planes, restated from the kernel's layout (csrc/pm_planes.hpp)."""
    tw, th, fill = pm.planes_constants()
    nv = 2 if prm.left_right_check else 1
    zero = dict.fromkeys(("launched", "stage", "patch", "window", "state_f16", "tile_w", "tile_h", "grid_x", "grid_y",
                          "lds_bytes", "rw", "margin", "fast_fill", "ref_regs", "tap_class"), 0)
    if stage == VIEW and nv == 1:
        return zero
    if stage == VIEW_REFINE and nv == 1:
        stage = REFINE
    P, window, md = prm.patch_w[0], prm.plane_window, prm.max_disp
    margin = slope_margin(prm)
    TW, TH = tw[stage], th[stage]
    rw = TW + 2 * (P // 2) + md + 2 * margin + 2
    TR, LW = TH + P - 1, TW + P - 1
    nref = ((8 if window == CHECKER else 4) * TR * ref_row_dwords(LW, window) + 1) & ~1
    words = 2 * nref + 2 * TR * rw + 4 + (3 * (TH + 2) * (TW + 2) if stage == SPATIAL else 0)
    return dict(launched=1, stage=stage, patch=P, window=window, state_f16=prm.state_dtype, tile_w=TW, tile_h=TH,
                grid_x=-(-cols // TW), grid_y=-(-rows // TH), lds_bytes=4 * words, rw=rw, margin=margin,
                fast_fill=int(cols % 2 == 0 and rw + 1 <= fill),
                ref_regs=int(stage == SPATIAL and window == CHECKER and pair_order(P)["shared"]),
                tap_class=tap_class(P, window))


def fill_limit_max_disp(pm, stage, patch=11, **kw):
    """The largest max_disp whose launches of `stage` still take the fast fill (even cols), from the plan."""
    lo, hi = 1, 4096
    assert pm.planes_plan(pparams(pm, patch=patch, max_disp=lo, **kw), stage, 16, 16)["fast_fill"] == 1
    assert pm.planes_plan(pparams(pm, patch=patch, max_disp=hi, **kw), stage, 16, 16)["fast_fill"] == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pm.planes_plan(pparams(pm, patch=patch, max_disp=mid, **kw), stage, 16, 16)["fast_fill"]:
            lo = mid
        else:
            hi = mid
    return lo


# ---- CPU: the plan ---------------------------------------------------------------------------------------------------------
def test_constants_and_tap_classes(pm):
    tw, th, fill = pm.planes_constants()
    assert len(tw) == 5 and len(th) == 5 and all(w % 64 == 0 and w > 0 for w in tw) and all(1 <= h <= 16 for h in th)
    assert tw[SPATIAL] == 2 * tw[REFINE] and len({tw[s] for s in WIDE_STAGES}) == 1 and fill % 128 == 0
    # the leftover groupings of PlPairOrder: 3 / 11, 5 / 13 and 7 / 15 share one each, 9 has its own (no odd leftover)
    classes = {}
    for P in WINDOWS:
        o = pair_order(P)
        classes.setdefault((o["RE"], o["RO"]), []).append(P)
        for window in (CHECKER, FULL):
            for f16 in (0, 1):
                for stage in STAGES:
                    rec = pm.planes_plan(pparams(pm, patch=P, f16=f16, plane_window=window, max_disp=32), stage, 20, 150)
                    assert rec["tap_class"] == tap_class(P, window), (P, window, rec)
                    assert rec["ref_regs"] == int(stage == SPATIAL and window == CHECKER and P in (3, 11)), (P, window, rec)
    assert classes == {(2, 1): [3, 11], (3, 2): [5, 13], (0, 3): [7, 15], (1, 0): [9]}
    assert {P for P in WINDOWS if pair_order(P)["shared"]} == {3, 11}
    assert len({tap_class(P, CHECKER) for P in WINDOWS}) == 4 and len({tap_class(P, FULL) for P in WINDOWS}) == 2
    assert {tap_class(P, CHECKER) for P in WINDOWS}.isdisjoint({tap_class(P, FULL) for P in WINDOWS})


def test_plan_equals_its_restatement(pm):
    tw, th, _ = pm.planes_constants()
    shapes = [(8, 8), (th[REFINE] + 5, 2 * tw[REFINE] + 2), (th[REFINE] + 5, 2 * tw[REFINE] + 3), (th[SPATIAL], tw[SPATIAL]),
              (th[SPATIAL] + 1, tw[SPATIAL] + 1), (720, 1280), (9, 257)]
    n = 0
    for P, window, f16, lr in itertools.product(WINDOWS, (CHECKER, FULL), (0, 1), (1, 0)):
        for md, smax in ((1, 1.0), (20, 1.0), (21, 0.3), (128, 1.0), (300, 0.5)):
            prm = pparams(pm, patch=P, f16=f16, plane_window=window, max_disp=md, plane_slope_max=smax, left_right_check=lr)
            for stage in STAGES:
                for rows, cols in shapes:
                    assert pm.planes_plan(prm, stage, rows, cols) == expected_plan(pm, prm, stage, rows, cols), \
                        (P, window, f16, lr, md, smax, stage, rows, cols)
                    n += 1
    assert n == 7 * 2 * 2 * 2 * 5 * 5 * len(shapes)


def test_fast_fill_flips_where_the_tile_row_passes_the_strips(pm):
    tw, _, fill = pm.planes_constants()
    for stage in STAGES:
        md = fill_limit_max_disp(pm, stage)
        for k, fast in ((md, 1), (md + 1, 0)):
            prm = pparams(pm, max_disp=k)
            rec = pm.planes_plan(prm, stage, 16, 130)
            assert rec["fast_fill"] == fast and (rec["rw"] + 1 <= fill) == bool(fast), (stage, k, rec)
            assert pm.planes_plan(prm, stage, 16, 131)["fast_fill"] == 0      # an odd width never
        assert pm.planes_plan(pparams(pm, max_disp=md), stage, 16, 130)["rw"] + 1 == fill
    # window 11, slope_max 1: 64-wide tiles up to max_disp 411, the 128-wide ones of the spatial stage up to 347
    assert (tw[REFINE], tw[SPATIAL]) != (64, 128) or \
        (fill_limit_max_disp(pm, REFINE), fill_limit_max_disp(pm, SPATIAL)) == (411, 347)


def test_lds_bytes_and_the_create_time_limit(pm):
    # what fits: the widest stage of every shipped configuration of tests/test_planes.py; what does not: 15 / 1024
    for patch, md, fits in ((11, 64, True), (11, 300, True), (15, 40, True), (5, 128, True), (15, 1024, False)):
        for window in (CHECKER, FULL):
            prm = pparams(pm, patch=patch, max_disp=md, plane_window=window)
            rec = pm.planes_plan(prm, SPATIAL, 64, 64)
            assert rec == expected_plan(pm, prm, SPATIAL, 64, 64)
            assert (rec["lds_bytes"] <= K_CHAIN_LDS_MAX) == fits, rec
            assert rec["lds_bytes"] >= max(pm.planes_plan(prm, s, 64, 64)["lds_bytes"] for s in STAGES)   # the widest


def test_plan_hook_refuses_what_it_cannot_plan(pm):
    import ctypes as C
    lib = pm.load()
    out = pm.PmDebugPlanesVariant()
    good = pparams(pm)
    assert lib.pm_debug_planes_plan(C.byref(good), SPATIAL, 8, 8, C.byref(out)) == pm.PM_OK and out.launched == 1
    for prm, stage, rows, cols in ((good, -1, 8, 8), (good, 5, 8, 8), (good, INIT, 0, 8), (good, INIT, 8, 0),
                                   (pm.default_params(0), INIT, 8, 8), (pparams(pm, patch=4), INIT, 8, 8),
                                   (pparams(pm, patch=17), INIT, 8, 8)):
        C.memset(C.byref(out), 0x5a, C.sizeof(out))
        assert lib.pm_debug_planes_plan(C.byref(prm), stage, rows, cols, C.byref(out)) == pm.PM_ERR_INVALID_ARG
        assert bytes(out) == bytes(C.sizeof(out))
    assert lib.pm_debug_planes_plan(None, INIT, 8, 8, C.byref(out)) == pm.PM_ERR_INVALID_ARG
    assert lib.pm_debug_planes_plan(C.byref(good), INIT, 8, 8, None) == pm.PM_ERR_INVALID_ARG
    assert lib.pm_debug_planes_last(None, C.byref(out)) == pm.PM_ERR_INVALID_ARG
    # one view: view propagation launches nothing, the fused stage is the refinement
    one = pparams(pm, left_right_check=0)
    assert not any(pm.planes_plan(one, VIEW, 8, 8).values())
    assert pm.planes_plan(one, VIEW_REFINE, 8, 8) == pm.planes_plan(one, REFINE, 8, 8)
    assert pm.planes_plan(one, REFINE, 8, 8)["stage"] == REFINE


def test_the_plan_compiles_without_hip_and_walks_its_grid_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/planes_plan_main.cpp: csrc/pm_planes_plan.hpp through g++ (no HIP header in reach) with AddressSanitizer
    and UBSan, over stages, windows, state types, disparity ranges and sizes from 1 x 1 on."""
    import subprocess
    from cpp_build import build_host_kernel
    exe = build_host_kernel(tmp_path / "planes_plan_main", "planes_plan_main.cpp", compiler=("g++",),
                            flags=("-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.endswith(" 0 broken\n"), (r.stdout, r.stderr)


def test_the_definitions_wrapper_refuses_images_below_the_rule(oracle):
    rng = np.random.default_rng(0)
    for rows, cols in ((1, 1), (7, 64), (64, 7), (5, 257)):
        img = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
        with pytest.raises(ValueError, match="too small"):
            oracle.planes_match(oracle.planes_params(n_iters=1, patch=3, max_disp=1), img, img)
    img = rng.integers(0, 256, (8, 8), dtype=np.uint8)
    dl, dr = oracle.planes_match(oracle.planes_params(n_iters=1, patch=15, max_disp=16), img, img)
    assert np.isfinite(dl).all() and np.isfinite(dr).all() and (dl >= 0).all() and (dl <= 7).all()


def test_finish_of_the_definition_is_the_end_of_its_match(oracle):
    """pmo_planes_finish is the code pmo_planes_match ends with: maps of the returned planes == the returned maps."""
    l, r = F.random_pair(16, 40, seed=1)
    for lr in (1, 0):
        p = oracle.planes_params(n_iters=2, patch=5, max_disp=12, left_right_check=lr, nthreads=2)
        dl, dr, planes = oracle.planes_match(p, l, r, want_planes=True)
        ov = oracle.PlanesViews(l, r)
        for v in range(2 if lr else 1):
            ov.planes[v][...] = planes[v]
        fl, fr = ov.finish(p)
        assert_same(fl, dl, "left map")
        if lr:
            assert_same(fr, dr, "right map")
            assert (dl == 0).any() and (dl != planes[0][2]).any()   # the mask did something


# ---- CPU: the fields reach the branches they claim ------------------------------------------------------------------------
E_ROWS_EXTRA, E_SHIFT, E_MAX_DISP = 5, 3, 24


def crafted_shape(pm):
    tw, th, _ = pm.planes_constants()
    # two tiles in y, two spatial tiles / three wide ones in x; odd; the windows of the pixels either side of the tile
    # border stay inside the image, where the true plane of a shifted texture costs 0
    return th[SPATIAL] + E_ROWS_EXTRA, tw[SPATIAL] + 19


def test_fields_reach_the_branches_they_claim(pm, oracle):
    tw, th, _ = pm.planes_constants()
    rows, cols = crafted_shape(pm)
    # spatial: candidates below 0, above min(max_disp, x), identical ones, and a planted plane across a border each way
    st, planted = F.spatial_field(rows, cols, tw[SPATIAL], th[SPATIAL], E_SHIFT, E_MAX_DISP)
    n = F.spatial_branch_counts(st, planted, tw[SPATIAL], th[SPATIAL], E_MAX_DISP, E_SHIFT)
    assert all(v > 0 for v in n.values()), n
    # ... and with the definition: after the two colour passes every pixel next to a planted one holds the true plane
    l, r = F.shifted_texture(rows, cols, E_SHIFT)
    op = oracle.planes_params(patch=11, max_disp=E_MAX_DISP, nthreads=2)
    ov = oracle.PlanesViews(l, r)
    assert ov.cost(op, 0, tw[SPATIAL], 3, 0.0, 0.0, float(E_SHIFT)) == 0.0
    ov.planes[0][...] = st
    took = {}
    for colour in (0, 1):
        before = ov.planes[0].copy()
        ov.spatial(op, 0, colour)
        changed = np.argwhere((ov.planes[0][2] != before[2]) & (ov.planes[0][2] == E_SHIFT) & (ov.planes[0][3] == 0))
        took[colour] = {(int(x), int(y)) for y, x in changed}
        assert all((x + y) % 2 == colour for x, y in took[colour]), "a pixel of the other colour changed"
    for x, y in planted:
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            assert (x + dx, y + dy) in took[(x + dx + y + dy) % 2], ((x, y), (dx, dy))
    # view propagation: ties of xo at even and odd k, 1 - a_other == 0.25, the float below it, 0, xo clamped on both sides
    for into in (0, 1):
        n = F.view_branch_counts(F.view_fields(rows, cols, into, E_SHIFT), into)
        assert all(v > 0 for v in n.values()), (into, n)
        sts = F.view_fields(rows, cols, into, E_SHIFT)
        for v in range(2):
            ov.planes[v][...] = sts[v]
        before = ov.planes[into].copy()
        ov.view_prop(op, into)
        assert ((ov.planes[into][3] != before[3]).sum() > 50) and (ov.planes[into][3] == F.HUGE).sum() > 50   # both outcomes
    # seeds: every special value, refused and clamped ones, column 0 -- in the coordinates of either view
    seeds = F.special_seed_map(rows, cols, E_MAX_DISP)
    for view_map in (seeds, seeds[:, ::-1]):
        n = F.seed_branch_counts(view_map, E_MAX_DISP)
        assert all(v > 0 for v in n.values()), n
    # refinement: the first step of at least some pixels leaves [0, zmax] on either side, and clamps a slope
    st = F.refine_field(rows, cols, 1.0, E_MAX_DISP)
    below = above = clamped = 0
    for y in range(0, rows, 3):
        for x in range(0, cols, 5):
            u = [np.float32(np.int32(np.uint32(oracle.planes_rand(op.seed, 1, 0, 0, 0, d, x, y)))) * np.float32(2.0 ** -31)
                 for d in range(3)]
            nz = np.float32(st[2, y, x] + np.float32(op.refine_amp[0]) * u[0])
            below += nz < 0
            above += nz > min(E_MAX_DISP, x)
            clamped += abs(np.float32(st[0, y, x] + np.float32(op.refine_amp[0] * op.slope_per_disp) * u[1])) > 1.0
    assert below > 0 and above > 0 and clamped > 0, (below, above, clamped)
    # f16: written values the state does not hold, and disparities whose rounding reaches min(max_disp, x)
    st = F.f16_field(rows, cols, E_MAX_DISP)
    q = F.as_f16_state(st)
    xs = np.arange(cols, dtype=np.float32)[None, :]
    assert ((q[:3] != st[:3]).mean() > 0.5) and ((q[2] == np.minimum(E_MAX_DISP, xs)) & (st[2] < q[2])).sum() > 0
    # finish: |dl - dr| == lr_tol, the floats around it, ties of the target column at even and odd k
    n = F.finish_branch_counts(*F.finish_states(rows, cols, 1.0, E_MAX_DISP), 1.0)
    assert all(v > 0 for v in n.values()), n


# ---- GPU: the runner ---------------------------------------------------------------------------------------------------------
SEEN = set()     # (stage, P, window shape, state type, fast_fill) of every record of every case


def once(fn):
    """A case runs once per session, pass or fail: the coverage test at the end of the file calls every case, so that it
    holds under a -k selection too, and must neither repeat the work nor report a failed case a second time."""
    done = set()

    @functools.wraps(fn)
    def wrapper(pm, oracle, *args):
        if args not in done:
            done.add(args)
            fn(pm, oracle, *args)
    return wrapper


def case_id(case):
    return "-".join("x".join(map(str, a)) if isinstance(a, tuple) else str(a) for a in case)


def mirror_step(ovs, op, nv, stage, arg):
    """The definition's side of pm_planes_step(stage, arg)."""
    for ov in ovs:
        if stage == SPATIAL:
            for v in range(nv):
                ov.spatial(op, v, arg)
        elif stage == VIEW:
            if nv == 2:
                ov.view_prop(op, arg)
        elif stage == REFINE:
            for v in range(nv):
                ov.refine(op, v, arg)
        else:
            v, it = arg & 1, arg >> 1
            if v < nv:
                if nv == 2:
                    ov.view_prop(op, v)
                ov.refine(op, v, it)


def run_stages(pm, oracle, prm, pairs, steps, seeds=None, states=None, expect=None, what="", finish=False, max_shape=None):
    """pm_planes_begin on `pairs` [(left, right), ...] (+ seeds [(seed_l, seed_r), ...] in image coordinates), optionally
    pm_planes_write of `states` [view 0, view 1] into every pair, then every (stage, arg) of `steps`; after each launch the
    record against the plan and expect(record, asked stage, what), and every plane of every view of every pair against the
    definition.  finish: pm_planes_finish against the definition's.  Returns the records."""
    import torch
    dev = torch.device("cuda:0")
    rows, cols = pairs[0][0].shape
    n, nv, f16 = len(pairs), (2 if prm.left_right_check else 1), prm.state_dtype == 1
    op = oparams(oracle, prm)
    up = lambda arrs, dt: torch.from_numpy(np.stack([np.ascontiguousarray(a) for a in arrs])).to(dev).to(dt).contiguous()
    L, R = up([p[0] for p in pairs], torch.uint8), up([p[1] for p in pairs], torch.uint8)
    SL = up([s[0] for s in seeds], torch.float32) if seeds else None
    SR = up([s[1] for s in seeds], torch.float32) if seeds else None
    torch.cuda.synchronize()   # the uploads run on torch's stream, the stages on the handle's
    ovs = [oracle.PlanesViews(l, r) for l, r in pairs]
    records = []

    def check(e, stage, arg):
        rec = e.debug_planes_last()
        tag = f"{what}: stage {stage} arg {arg}"
        assert rec == pm.planes_plan(prm, stage, rows, cols), (tag, rec)          # what ran is what was planned
        if rec["launched"]:
            assert (rec["patch"], rec["window"], rec["state_f16"]) == (prm.patch_w[0], prm.plane_window, prm.state_dtype), tag
            SEEN.add((rec["stage"], rec["patch"], rec["window"], rec["state_f16"], rec["fast_fill"]))
        if expect:
            expect(rec, stage, tag)
        records.append(rec)
        for i, ov in enumerate(ovs):
            for v in range(nv):
                got = e.planes_read(i, v)
                for k in range(4):
                    assert_same(got[k], ov.planes[v][k], f"{tag}: pair {i} view {v} {NAMES[k]}")

    mr, mc = max_shape or (rows, cols)
    with pm.Engine(prm, max_rows=mr, max_cols=mc, max_batch=n) as e:
        e.planes_begin(n, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr() if seeds else None,
                       SR.data_ptr() if seeds else None)
        for i, ov in enumerate(ovs):
            for v in range(nv):
                seed = None
                if seeds:
                    seed = seeds[i][0] if v == 0 else seeds[i][1][:, ::-1]    # the right map comes in right-image coordinates
                ov.init(op, v, seed)
        check(e, INIT, 0)
        if states is not None:
            for i, ov in enumerate(ovs):
                for v in range(nv):
                    e.planes_write(i, v, states[v])
                    ov.planes[v][...] = F.as_f16_state(states[v]) if f16 else states[v]   # an f16 state rounds what it is given
                    got = e.planes_read(i, v)
                    for k in range(4):
                        assert_same(got[k], ov.planes[v][k], f"{what}: written state, pair {i} view {v} {NAMES[k]}")
        for stage, arg in steps:
            e.planes_step(stage, arg)
            mirror_step(ovs, op, nv, stage, arg)
            check(e, stage, arg)
        if finish:
            DL = torch.full((n, rows, cols), -7.0, dtype=torch.float32, device=dev)
            DR = torch.full((n, rows, cols), -7.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()   # the sentinel fill runs on torch's stream, the stage on the handle's
            e.planes_finish(DL.data_ptr(), DR.data_ptr() if nv == 2 else None)
            e.synchronize()
            for i, ov in enumerate(ovs):
                wl, wr = ov.finish(op)
                assert_same(DL[i].cpu().numpy(), wl, f"{what}: finish, pair {i} left map")
                if nv == 2:
                    assert_same(DR[i].cpu().numpy(), wr, f"{what}: finish, pair {i} right map")
    return records


def full_sequence(iters_spatial=2):
    """init (implied), the colour passes of `iters_spatial` iterations, view propagation into 0 and 1, refinement, then
    the fused view propagation + refinement of iteration 1 for both views -- as Match() launches it."""
    steps = [(SPATIAL, c + 2 * it) for it in range(iters_spatial) for c in (0, 1)]
    return steps + [(VIEW, 0), (VIEW, 1), (REFINE, 0), (VIEW_REFINE, 2), (VIEW_REFINE, 3)]


def sparse_seeds(left, seed, value=3.0):
    rng = np.random.default_rng(6000 + seed)
    sl = np.where(rng.random(left.shape) < 0.15, value, 0.0).astype(np.float32)
    sr = np.where(rng.random(left.shape) < 0.15, value, 0.0).astype(np.float32)
    return sl, sr


def expect_variant(pm, prm, rows, cols, fast=None):
    """The record of every launch of a case: the instantiation of the parameters, the grid of the shape, the fill path of
    the width (fast: {stage: 0 / 1} where the case is about it), the register window and the tap class of the window."""
    P, window = prm.patch_w[0], prm.plane_window

    def expect(rec, asked, tag):
        assert rec["launched"] == 1 and rec["stage"] == asked, (tag, rec)
        assert (rec["grid_x"], rec["grid_y"]) == (-(-cols // rec["tile_w"]), -(-rows // rec["tile_h"])), (tag, rec)
        assert rec["ref_regs"] == int(asked == SPATIAL and window == CHECKER and P in (3, 11)), (tag, rec)
        assert rec["tap_class"] == tap_class(P, window), (tag, rec)
        if fast is not None:
            assert rec["fast_fill"] == fast[asked], (tag, rec)
    return expect


# ---- a. every (window, window shape, state type) at a partial-tile shape ----------------------------------------------------
# rows = tile height + 5; widths = two wide tiles + 2 (even: the fast fill) and + 3 (odd: entry by entry) -- one spatial tile
# and a bit.  max_disp 20 and 21 at the even width: both parities of the tile's first target column (the fast fill loads
# from the even column at or below it), 21 at the odd width.
A_COMBOS = (("even", 20), ("odd", 21), ("even", 21))
A_CASES = [(P, window, f16, combo) for P in WINDOWS for window in (CHECKER, FULL) for f16 in (0, 1) for combo in range(3)]


@once
def check_partial_tiles(pm, oracle, P, window, f16, combo):
    tw, th, _ = pm.planes_constants()
    parity, md = A_COMBOS[combo]
    rows = max(th) + 5
    cols = 2 * tw[REFINE] + (2 if parity == "even" else 3)
    assert cols % 2 == (0 if parity == "even" else 1) and rows >= MIN_SIZE
    l, r = F.random_pair(rows, cols, seed=P)
    options = itertools.product((False, True), (FOUR, TWO)) if combo < 2 else ((False, FOUR), (True, TWO))
    for seeded, neighbours in options:
        prm = pparams(pm, patch=P, f16=f16, plane_window=window, plane_neighbours=neighbours, max_disp=md)
        base = expect_variant(pm, prm, rows, cols, fast={s: int(parity == "even") for s in STAGES})

        def expect(rec, asked, tag):
            base(rec, asked, tag)
            # partial tiles on both axes, more than one block on both
            assert cols % rec["tile_w"] and rows % rec["tile_h"] and rec["grid_x"] >= 2 and rec["grid_y"] >= 2, (tag, rec)
        run_stages(pm, oracle, prm, [(l, r)], full_sequence(), seeds=[sparse_seeds(l, P)] if seeded else None, expect=expect,
                   what=f"a: window {P} shape {window} f16 {f16} {cols}x{rows} max_disp {md} seeded {seeded} neighbours {neighbours}")


@gpu
@pytest.mark.parametrize("case", A_CASES, ids=case_id)
def test_every_instantiation_at_a_partial_tile_shape(pm, oracle, case):
    check_partial_tiles(pm, oracle, *case)


# ---- b. tile edges -----------------------------------------------------------------------------------------------------------
# rows in {tile height - 1, tile height, + 1} x cols in {w - 1, w, w + 1} for the wide tile and the spatial tile; windows 11
# (register window, shared leftover group) and 9 (its own grouping), checkerboard, f32.  Rows below the library's minimum
# belong to test_images_below_the_rule_are_refused.
def b_shapes(pm):
    tw, th, _ = pm.planes_constants()
    return [(r, w + dw, w) for r in (th[SPATIAL] - 1, th[SPATIAL], th[SPATIAL] + 1) for w in (tw[REFINE], tw[SPATIAL])
            for dw in (-1, 0, 1)]


B_CASES = [(P, k) for P in (11, 9) for k in range(18)]


@once
def check_tile_edges(pm, oracle, P, k):
    rows, cols, w = b_shapes(pm)[k]
    if rows < MIN_SIZE:
        return check_refused(pm, oracle, rows, cols)
    prm = pparams(pm, patch=P, max_disp=24)
    base = expect_variant(pm, prm, rows, cols)
    seen_class = set()

    def expect(rec, asked, tag):
        base(rec, asked, tag)
        if rec["tile_w"] == w:   # the stages whose tile the width is about: one column short, exact, one column over
            assert cols - w in (-1, 0, 1) and rec["grid_x"] == (2 if cols > w else 1), (tag, rec)
            assert abs(rows - rec["tile_h"]) <= 1 and rec["grid_y"] == (2 if rows > rec["tile_h"] else 1), (tag, rec)
            seen_class.add(asked)
    l, r = F.random_pair(rows, cols, seed=k)
    run_stages(pm, oracle, prm, [(l, r)], full_sequence(1), seeds=[sparse_seeds(l, k)], expect=expect,
               what=f"b: window {P} {cols}x{rows}")
    assert seen_class, "no stage has a tile of the width the case is about"


@gpu
@pytest.mark.parametrize("case", B_CASES, ids=case_id)
def test_tile_edges(pm, oracle, case):
    check_tile_edges(pm, oracle, *case)


# ---- c. the smallest images, below a tile and below the window -------------------------------------------------------------
C_SHAPES = [(8, 8), (8, 9), (9, 8), (8, 15), (8, 257)]      # (rows, cols): the rule's minimum, both parities, odd and wide
C_CASES = [(P, md, f16, s) for P in (3, 9, 15) for md in (1, 16) for f16 in (0, 1) for s in range(len(C_SHAPES))]
REFUSED_SHAPES = [(1, 1), (1, 2), (2, 1), (1, 7), (3, 5), (5, 257), (7, 64), (7, 129), (64, 7)]


@once
def check_small_images(pm, oracle, P, md, f16, s):
    rows, cols = C_SHAPES[s]
    prm = pparams(pm, patch=P, f16=f16, max_disp=md, iters=2)
    l, r = F.random_pair(rows, cols, seed=s, max_shift=1 if md == 1 else 6)
    tw, th, _ = pm.planes_constants()
    assert rows >= MIN_SIZE and cols >= MIN_SIZE and (min(rows, cols) < P or P == 3)        # below the window (but 3)
    assert rows <= min(th) + 1 and (cols < min(tw) or cols > 2 * max(tw))                  # below a tile, or a row of them
    run_stages(pm, oracle, prm, [(l, r)], full_sequence(1), expect=expect_variant(pm, prm, rows, cols), finish=True,
               what=f"c: window {P} {cols}x{rows} max_disp {md} f16 {f16}")
    want = oracle.planes_match(oparams(oracle, prm), l, r)
    with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:
        got = e.match(l, r)
    assert_same(got[0], want[0], f"c: Match() {cols}x{rows} left map")
    assert_same(got[1], want[1], f"c: Match() {cols}x{rows} right map")


@gpu
@pytest.mark.parametrize("case", C_CASES, ids=case_id)
def test_smallest_images(pm, oracle, case):
    check_small_images(pm, oracle, *case)


@once
def check_refused(pm, oracle, rows, cols):
    """Below 8 x 8: PM_ERR_INVALID_ARG from pm_planes_begin (which names itself) and from Match(), nothing launched, and the
    handle goes on to do an image it takes -- bit-identical to the definition."""
    import torch
    dev = torch.device("cuda:0")
    prm = pparams(pm, patch=3, max_disp=4, iters=1)
    img = torch.zeros((max(rows, 8), max(cols, 8)), dtype=torch.uint8, device=dev)
    l, r = F.random_pair(8, 12, seed=rows + cols)
    want = oracle.planes_match(oparams(oracle, prm), l, r)
    with pytest.raises(ValueError):
        oracle.planes_match(oparams(oracle, prm), np.zeros((rows, cols), np.uint8), np.zeros((rows, cols), np.uint8))
    with pm.Engine(prm, max_rows=max(rows, 8), max_cols=max(cols, 12)) as e:
        with pytest.raises(pm.PmError) as err:
            e.planes_begin(1, img.data_ptr(), img.data_ptr(), rows, cols)
        assert err.value.status == pm.PM_ERR_INVALID_ARG and "pm_planes_begin" in str(err.value), str(err.value)
        assert not any(e.debug_planes_last().values())
        with pytest.raises(pm.PmError):                       # no state to step on
            e.planes_step(pm.PM_PL_SPATIAL, 0)
        with pytest.raises(pm.PmError) as err:
            e.match(np.zeros((rows, cols), np.uint8), np.zeros((rows, cols), np.uint8))
        assert err.value.status == pm.PM_ERR_INVALID_ARG
        got = e.match(l, r)
        assert_same(got[0], want[0], "the handle after a refusal, left map")
        assert_same(got[1], want[1], "the handle after a refusal, right map")


@gpu
@pytest.mark.parametrize("shape", REFUSED_SHAPES, ids=case_id)
def test_images_below_the_rule_are_refused(pm, oracle, shape):
    check_refused(pm, oracle, *shape)


# ---- d. the fill switch ------------------------------------------------------------------------------------------------------
# Even cols.  Per tile class (the wide stages, the spatial stage): the last max_disp with the fast fill and the first
# without (window 11, slope_max 1: 411 / 412 and 347 / 348), and around every 128-entry strip boundary of the fast fill the
# max_disp whose tile row ends one entry before it, on it and one entry behind it: strip t loads where 128 t < rw + (first
# target column odd), and that parity changes with max_disp, so the three straddle the strip's first entry.  All from the plan.
def d_cases(pm):
    """[(tile class, max_disp, fast_fill, rw or None)]"""
    tw, th, fill = pm.planes_constants()
    cases = []
    for cls, stage in (("wide", REFINE), ("spatial", SPATIAL)):
        lim = fill_limit_max_disp(pm, stage)
        cases += [(cls, lim, 1, None), (cls, lim + 1, 0, None)]
        rw0 = pm.planes_plan(pparams(pm, max_disp=1), stage, 16, 16)["rw"] - 1      # rw = rw0 + max_disp
        cases += [(cls, b + extra - rw0, 1, b + extra) for b in range(128, fill, 128) for extra in (-1, 0, 1)
                  if b + extra - rw0 >= 1]
    return cases


D_CASES = list(range(19))


@once
def check_fill_switch(pm, oracle, k):
    tw, th, fill = pm.planes_constants()
    cases = d_cases(pm)
    assert len(cases) == len(D_CASES), cases      # (retuned constants: adjust D_CASES to the new list, drop nothing)
    cls, md, fast, rw = cases[k]
    rows, cols = th[SPATIAL] + 5, 2 * tw[REFINE] + 2
    assert cols % 2 == 0
    prm = pparams(pm, max_disp=md)
    about = (SPATIAL,) if cls == "spatial" else WIDE_STAGES

    def expect(rec, asked, tag):
        if asked in about:
            assert rec["fast_fill"] == fast and (rec["rw"] + 1 <= fill) == bool(fast), (tag, rec)
            assert rw is None or rec["rw"] == rw, (tag, rec)
    l, r = F.random_pair(rows, cols, seed=k)
    run_stages(pm, oracle, prm, [(l, r)], full_sequence(1), seeds=[sparse_seeds(l, k)], expect=expect,
               what=f"d: {cls} tiles, max_disp {md}")


@gpu
@pytest.mark.parametrize("k", D_CASES)
def test_fill_switch_and_strip_boundaries(pm, oracle, k):
    check_fill_switch(pm, oracle, k)


# ---- e. crafted states through pm_planes_write -----------------------------------------------------------------------------
E_CASES = [(P, f16, kind) for P in (11, 9, 5) for f16 in (0, 1) for kind in ("spatial4", "spatial2", "view0", "view1", "refine", "f16values")]


@once
def check_crafted(pm, oracle, P, f16, kind):
    tw, th, _ = pm.planes_constants()
    rows, cols = crafted_shape(pm)
    l, r = F.shifted_texture(rows, cols, E_SHIFT)
    neighbours = TWO if kind == "spatial2" else FOUR
    prm = pparams(pm, patch=P, f16=f16, max_disp=E_MAX_DISP, plane_neighbours=neighbours)
    what = f"e: {kind}, window {P}, f16 {f16}"
    expect = expect_variant(pm, prm, rows, cols)
    if kind.startswith("spatial"):
        st, _ = F.spatial_field(rows, cols, tw[SPATIAL], th[SPATIAL], E_SHIFT, E_MAX_DISP)
        steps = [(SPATIAL, a) for a in (0, 1, 2, 3)]           # both colours of an even and an odd iteration
        run_stages(pm, oracle, prm, [(l, r)], steps, states=[st, st[:, :, ::-1].copy()], expect=expect, what=what)
        run_stages(pm, oracle, prm, [(l, r)], steps[::-1], states=[st, st], expect=expect, what=what + " (odd iteration first)")
    elif kind.startswith("view"):
        into = int(kind[-1])
        sts = F.view_fields(rows, cols, into, E_SHIFT)
        run_stages(pm, oracle, prm, [(l, r)], [(VIEW, into), (VIEW, 1 - into)], states=sts, expect=expect, what=what)
        run_stages(pm, oracle, prm, [(l, r)], [(VIEW_REFINE, into), (VIEW_REFINE, 2 + 1 - into)], states=sts, expect=expect,
                   what=what + " (fused)")
    elif kind == "refine":
        smax = float(np.float16(prm.plane_slope_max)) if f16 else prm.plane_slope_max
        st = F.refine_field(rows, cols, smax, E_MAX_DISP)
        run_stages(pm, oracle, prm, [(l, r)], [(REFINE, 0), (REFINE, 5), (VIEW_REFINE, 2), (VIEW_REFINE, 7)], states=[st, st],
                   expect=expect, what=what)
    else:
        st = F.f16_field(rows, cols, E_MAX_DISP)
        run_stages(pm, oracle, prm, [(l, r)], full_sequence(), states=[st, st[:, ::-1].copy()], expect=expect, finish=True, what=what)


@gpu
@pytest.mark.parametrize("case", E_CASES, ids=case_id)
def test_crafted_states(pm, oracle, case):
    check_crafted(pm, oracle, *case)


# ---- f. seeds at initialisation -----------------------------------------------------------------------------------------------
F_CASES = [(f16, sparse) for f16 in (0, 1) for sparse in (0, 1)]


@once
def check_special_seeds(pm, oracle, f16, sparse_init):
    """NaN, +-inf, negatives, -0, a subnormal, values above max_disp and above the column, column 0 included, for both
    views (the right map in right-image coordinates); with sparse_init = 1 the caller's maps still are the seeds."""
    rows, cols = crafted_shape(pm)
    l, r = F.random_pair(rows, cols, seed=9)
    # (a handle with the device seeder wants max_disp >= the seeder's template width)
    md = max(E_MAX_DISP, pm.default_params(0).templ_cols) if sparse_init else E_MAX_DISP
    sl = F.special_seed_map(rows, cols, md, seed=1)
    sr = F.special_seed_map(rows, cols, md, seed=2)
    for view_map in (sl, sr[:, ::-1]):
        n = F.seed_branch_counts(view_map, md)
        assert all(v > 0 for v in n.values()), n
    kw = dict(sparse_init=1, init_dilate_factor=2) if sparse_init else {}
    prm = pparams(pm, patch=7, f16=f16, max_disp=md, **kw)
    run_stages(pm, oracle, prm, [(l, r)], [(SPATIAL, 0), (SPATIAL, 1)], seeds=[(sl, sr)],
               expect=expect_variant(pm, prm, rows, cols), what=f"f: special seeds, f16 {f16}, sparse_init {sparse_init}",
               max_shape=(96, 256) if sparse_init else None)


@gpu
@pytest.mark.parametrize("case", F_CASES, ids=case_id)
def test_special_seed_values(pm, oracle, case):
    check_special_seeds(pm, oracle, *case)


# ---- g. pm_planes_finish on written states ------------------------------------------------------------------------------------
G_CASES = [(f16, lr_tol) for f16 in (0, 1) for lr_tol in (1.0, 0.5)]


@once
def check_finish(pm, oracle, f16, lr_tol):
    rows, cols = crafted_shape(pm)
    l, r = F.random_pair(rows, cols, seed=4)
    st0, st1 = F.finish_states(rows, cols, lr_tol, E_MAX_DISP)
    if not f16:
        n = F.finish_branch_counts(st0, st1, lr_tol)
        assert all(v > 0 for v in n.values()), n
    prm = pparams(pm, patch=5, f16=f16, max_disp=E_MAX_DISP, plane_lr_tol=lr_tol)
    run_stages(pm, oracle, prm, [(l, r)], [], states=[st0, st1], finish=True, what=f"g: finish, f16 {f16}, lr_tol {lr_tol}")
    one = pparams(pm, patch=5, f16=f16, max_disp=E_MAX_DISP, plane_lr_tol=lr_tol, left_right_check=0)
    run_stages(pm, oracle, one, [(l, r)], [], states=[st0, st1], finish=True, what=f"g: finish with one view, f16 {f16}")


@gpu
@pytest.mark.parametrize("case", G_CASES, ids=case_id)
def test_finish_on_written_states(pm, oracle, case):
    check_finish(pm, oracle, *case)


# ---- h. three pairs through the stage API, and one view ---------------------------------------------------------------------------
H_CASES = [(P, f16, lr) for P in (11, 7) for f16 in (0, 1) for lr in (1, 0)]


@once
def check_pairs_and_views(pm, oracle, P, f16, lr):
    tw, th, _ = pm.planes_constants()
    rows, cols = th[SPATIAL] + 5, tw[SPATIAL] + 2
    pairs = [F.random_pair(rows, cols, seed=20 + i) for i in range(3)]
    seeds = [sparse_seeds(p[0], 20 + i) for i, p in enumerate(pairs)]
    prm = pparams(pm, patch=P, f16=f16, max_disp=20, left_right_check=lr)
    base = expect_variant(pm, prm, rows, cols)

    def expect(rec, asked, tag):
        if lr == 0 and asked == VIEW:
            assert not any(rec.values()), (tag, rec)          # a no-op: nothing launched, nothing recorded
        elif lr == 0 and asked == VIEW_REFINE:
            assert rec["launched"] == 1 and rec["stage"] == REFINE, (tag, rec)   # the refine kernel
        else:
            base(rec, asked, tag)
    steps = full_sequence() if lr else [(SPATIAL, 0), (SPATIAL, 1), (VIEW, 0), (VIEW, 1), (REFINE, 0), (VIEW_REFINE, 2)]
    # run_stages compares every pair with ITS OWN definition run: each pair equals its single
    run_stages(pm, oracle, prm, pairs, steps, seeds=seeds, expect=expect, finish=True, what=f"h: 3 pairs, window {P}, f16 {f16}, lr {lr}")
    if lr == 0:
        with pm.Engine(prm, max_rows=rows, max_cols=cols) as e:   # view 1 of the fused stage: not a view of this handle
            import torch
            L = torch.from_numpy(pairs[0][0]).to("cuda:0").contiguous()
            R = torch.from_numpy(pairs[0][1]).to("cuda:0").contiguous()
            e.planes_begin(1, L.data_ptr(), R.data_ptr(), rows, cols)
            before = e.planes_read(0, 0)
            e.planes_step(pm.PM_PL_VIEW_REFINE, 3)
            assert not any(e.debug_planes_last().values())
            assert_same(e.planes_read(0, 0), before, "a stage for a view the handle does not have")


@gpu
@pytest.mark.parametrize("case", H_CASES, ids=case_id)
def test_three_pairs_and_one_view(pm, oracle, case):
    check_pairs_and_views(pm, oracle, *case)


@gpu
def test_create_refuses_a_tile_beyond_the_lds_and_the_record_starts_empty(pm):
    with pytest.raises(pm.PmError) as err:
        pm.Engine(pparams(pm, patch=15, max_disp=1024), max_rows=64, max_cols=64)
    assert err.value.status == pm.PM_ERR_INVALID_ARG
    with pm.Engine(pparams(pm), max_rows=16, max_cols=16) as e:
        assert not any(e.debug_planes_last().values())


# ---- i. the cases together show every instantiation on both fill paths -------------------------------------------------------
@gpu
def test_the_cases_cover_every_instantiation(pm, oracle):
    for check, cases in ((check_partial_tiles, A_CASES), (check_tile_edges, B_CASES), (check_small_images, C_CASES),
                         (check_refused, REFUSED_SHAPES), (check_fill_switch, [(k,) for k in D_CASES]),
                         (check_crafted, E_CASES), (check_special_seeds, F_CASES), (check_finish, G_CASES),
                         (check_pairs_and_views, H_CASES)):
        for case in cases:
            check(pm, oracle, *case)   # returns at once where the case has run
    want = set(itertools.product(STAGES, WINDOWS, (FULL, CHECKER), (0, 1), (0, 1)))
    assert SEEN >= want, sorted(want - SEEN)
    assert {v[:4] for v in SEEN} == {v[:4] for v in want}, "a record names an instantiation the library does not hold"
