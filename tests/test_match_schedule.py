"""What one Match() call enqueues, route by route: the launches per kernel class of one profiled call, and its maps.

csrc/pm_match_plan.hpp::plan_match decides the route of a call (tests/test_match_plan.py pins those decisions on the
CPU); this module runs one call per route on the device with profiling on and asserts the EXACT number of brackets per
class (pm_profile.launches) -- DESIGN.md 6, "The routes of a Match()" -- and that the maps are the oracle's, or, where a
view seeds itself on the device, those of the same pairs matched one by one (as test_gpu_parity.py's self-seeded batch).

  I = patchmatch_iters, S = 5 seeder stages, s0 / s1 = 1 where view 0 / 1 seeds itself, K = ceil(n / 2) chunks, L lanes

  route                      prep  seed                  noise_cost  sweep_row = sweep_col  background  finalize
  A one stream (lr = 0)      2     1 + s0                I           2I                     1           1
  B BGR input (lr = 1)       2     1 + n S (s0 + s1)     2I          4I                     2           1
  C two streams (n <= 2)     4     n S (s0 + s1)         2I          4I                     2           1
  D chunks                   4K    K (s0 + s1)           2IK         4IK                    2K          K
  P planes                   1     s0 + s1               planes_init 1, planes_spatial 2IL, planes_view_refine 2IL, finalize 1

The pm_submit_* ring is left out: how its frames pair up depends on whether the device is still busy.
"""
import os

import numpy as np
import pytest

import oracle_lib as O
from conftest import assert_same, small_pair

if os.environ.get("PM_LIB"):   # another build of the library (a tuning build reads knobs that change the routes)
    pytest.skip("PM_LIB is set: the counts below are the shipped library's", allow_module_level=True)

pytestmark = pytest.mark.gpu

I, S = 2, 5
SEEDED_SHAPE, SELF_SHAPE, PLANES_SHAPE = (48, 80), (96, 160), (64, 96)
SEEDER = dict(sparse_init=1, max_features_per_frame=60, min_distance_btw_features=8, max_disp=48, templ_cols=15,
              templ_rows=7)   # test_gpu_parity.py::test_self_seeded_batch_on_lanes_equals_singles
CLASSES = ("prep", "seed", "noise_cost", "sweep_row", "sweep_col", "background", "finalize", "planes_init",
           "planes_spatial", "planes_view", "planes_refine", "planes_view_refine")


def counts(prep=0, seed=0, noise_cost=0, sweeps=0, background=0, finalize=0, **planes):
    want = dict.fromkeys(CLASSES, 0)
    want.update(prep=prep, seed=seed, noise_cost=noise_cost, sweep_row=sweeps, sweep_col=sweeps, background=background,
                finalize=finalize, **planes)
    return want


@pytest.fixture(scope="module")
def pairs(synth):
    """three pairs per shape, made once: (left, right, seed_l, seed_r, gt)"""
    return {shape: [small_pair(synth, 700 + i, shape[0], shape[1], n_points=25, dilate_factor=2) for i in range(3)]
            for shape in (SEEDED_SHAPE, SELF_SHAPE, PLANES_SHAPE)}


def scalar_params(pm, lr, self_seeded):
    kw = dict(SEEDER) if self_seeded else {}
    return pm.default_params(0, patch=3 if self_seeded else 5, patchmatch_iters=I, left_right_check=lr, **kw)


def singles(pm, prm, shape, prs, give_l, give_r):
    """every pair matched alone (route A or C at n = 1): what a self-seeded batch must reproduce slot by slot"""
    with pm.Engine(prm, max_rows=shape[0], max_cols=shape[1]) as e:
        out = [e.match(p[0], p[1], p[2] if give_l else None, p[3] if give_r else None) for p in prs]
    assert any((s[0] > 0).any() for s in out), "the seeder found nothing: the test would compare zeros"
    return out


def profiled_device_call(pm, prm, shape, lefts, rights, seeds_l, seeds_r, bgr=False):
    """one pm_match_device / pm_match_bgr_device on n pairs with profiling on -> (launches per class, left maps, right maps)"""
    import torch
    rows, cols = shape
    n = len(lefts)
    dev = torch.device("cuda:0")
    up = lambda arrs: torch.from_numpy(np.stack(arrs)).to(dev).contiguous() if arrs is not None else None
    L, R, SL, SR = up(lefts), up(rights), up(seeds_l), up(seeds_r)
    DL = torch.empty((n, rows, cols), dtype=torch.float32, device=dev)
    DR = torch.empty_like(DL) if prm.left_right_check else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    with pm.Engine(prm, max_rows=rows, max_cols=cols, max_batch=n) as e:
        e.profile_enable()
        call = e.match_bgr_device if bgr else e.match_device
        call(n, ptr(L), ptr(R), rows, cols, ptr(SL), ptr(SR), ptr(DL), ptr(DR))
        e.synchronize()
        got = {k: v[0] for k, v in e.profile_read().items()}
    return got, DL.cpu().numpy(), DR.cpu().numpy() if DR is not None else None


def check_maps(dl, dr, want, what):
    for i, (wl, wr) in enumerate(want):
        assert_same(dl[i], wl, f"{what}: pair {i}, left")
        if wr is not None:
            assert_same(dr[i], wr, f"{what}: pair {i}, right")


def scalar_case(pm, oracle, pairs, lr, n, give_l, give_r, want, what):
    self_seeded = not (give_l and give_r)
    shape = SELF_SHAPE if self_seeded else SEEDED_SHAPE
    prs = pairs[shape][:n]
    prm = scalar_params(pm, lr, self_seeded)
    got, dl, dr = profiled_device_call(pm, prm, shape, [p[0] for p in prs], [p[1] for p in prs],
                                       [p[2] for p in prs] if give_l else None, [p[3] for p in prs] if give_r else None)
    assert got == want, (what, got)
    if self_seeded:
        ref = singles(pm, prm, shape, prs, give_l, give_r)
    else:
        op = oracle.default_params(0, patch=5, n_iters=I, left_right_check=lr, nthreads=8)
        ref = [oracle.match(op, *p[:4]) for p in prs]
    check_maps(dl, dr, ref, what)


# ---- route A: one view, everything on the handle's stream -------------------------------------------------------------
@pytest.mark.parametrize("n, self_seeded", [(1, False), (3, False), (1, True), (3, True)])
def test_route_a_one_stream(pm, oracle, pairs, n, self_seeded):
    s0 = 1 if self_seeded else 0
    want = counts(prep=2, seed=1 + s0, noise_cost=I, sweeps=2 * I, background=1, finalize=1)
    scalar_case(pm, oracle, pairs, 0, n, not self_seeded, not self_seeded, want, f"route A, n = {n}")


# ---- route C: two views of up to two pairs, each view with its own head on its own stream ---------------------------
@pytest.mark.parametrize("n, self_seeded", [(1, False), (2, False), (1, True), (2, True)])
def test_route_c_two_streams(pm, oracle, pairs, n, self_seeded):
    s = 2 if self_seeded else 0
    want = counts(prep=4, seed=n * S * s, noise_cost=2 * I, sweeps=4 * I, background=2, finalize=1)
    scalar_case(pm, oracle, pairs, 1, n, not self_seeded, not self_seeded, want, f"route C, n = {n}")


# ---- route D: chunks of two pairs; the head runs aside exactly when a view seeds itself -------------------------------
@pytest.mark.parametrize("give_l, give_r", [(True, True), (False, False), (True, False)])
def test_route_d_chunks_through_match_device(pm, oracle, pairs, give_l, give_r):
    n, K = 3, 2
    s = (0 if give_l else 1) + (0 if give_r else 1)
    want = counts(prep=4 * K, seed=K * s, noise_cost=2 * I * K, sweeps=4 * I * K, background=2 * K, finalize=K)
    scalar_case(pm, oracle, pairs, 1, n, give_l, give_r, want, f"route D, seeds given: {give_l}, {give_r}")


@pytest.mark.parametrize("n", [2, 3])
def test_route_d_chunks_through_match_batch(pm, oracle, pairs, n):
    K = (n + 1) // 2
    prs = pairs[SEEDED_SHAPE][:n]
    prm = scalar_params(pm, 1, False)
    with pm.Engine(prm, max_rows=SEEDED_SHAPE[0], max_cols=SEEDED_SHAPE[1], max_batch=n) as e:
        e.profile_enable()
        dls, drs = e.match_batch([p[0] for p in prs], [p[1] for p in prs], [p[2] for p in prs], [p[3] for p in prs])
        got = {k: v[0] for k, v in e.profile_read().items()}
    assert got == counts(prep=4 * K, noise_cost=2 * I * K, sweeps=4 * I * K, background=2 * K, finalize=K), got
    op = oracle.default_params(0, patch=5, n_iters=I, nthreads=8)
    check_maps(dls, drs, [oracle.match(op, *p[:4]) for p in prs], f"match_batch, n = {n}")


# ---- route B: BGR input, one head for both views on the handle's stream, then the views on two streams ----------------
@pytest.mark.parametrize("n, self_seeded", [(1, False), (2, False), (1, True), (2, True)])
def test_route_b_bgr(pm, oracle, synth, pairs, n, self_seeded):
    shape = SELF_SHAPE if self_seeded else SEEDED_SHAPE
    prs = pairs[shape][:n]
    bl = [synth.to_bgr(p[0], 3 + i) for i, p in enumerate(prs)]   # inputs as in tests/test_enhance.py
    br = [synth.to_bgr(p[1], 7 + i) for i, p in enumerate(prs)]
    prm = scalar_params(pm, 1, self_seeded)
    s = 2 if self_seeded else 0
    got, dl, dr = profiled_device_call(pm, prm, shape, bl, br, None if self_seeded else [p[2] for p in prs],
                                       None if self_seeded else [p[3] for p in prs], bgr=True)
    assert got == counts(prep=2, seed=1 + n * S * s, noise_cost=2 * I, sweeps=4 * I, background=2, finalize=1), got
    # the enhancement's gray images (bit-identical on the device: tests/test_enhance.py), then the gray routes' references
    gray = [(O.stereo_ready(l)[1], O.stereo_ready(r)[1], p[2], p[3]) for l, r, p in zip(bl, br, prs)]
    if self_seeded:
        ref = singles(pm, prm, shape, gray, False, False)
    else:
        op = oracle.default_params(0, patch=5, n_iters=I, nthreads=8)
        ref = [oracle.match(op, *g) for g in gray]
    check_maps(dl, dr, ref, f"route B, n = {n}")


# ---- route P: plane mode, one head for all pairs, then one lane (n = 1) or two -----------------------------------------
@pytest.mark.parametrize("n, lanes", [(1, 1), (2, 2), (3, 2)])
@pytest.mark.parametrize("self_seeded", [False, True])
def test_route_p_planes(pm, oracle, pairs, n, lanes, self_seeded):
    prs = pairs[PLANES_SHAPE][:n]
    kw = dict(SEEDER, init_dilate_factor=2) if self_seeded else dict(max_disp=48)
    prm = pm.default_params(0, patch=7, patchmatch_iters=I, mode=pm.PM_MODE_PLANES, state_dtype=pm.PM_STATE_F32, **kw)
    got, dl, dr = profiled_device_call(pm, prm, PLANES_SHAPE, [p[0] for p in prs], [p[1] for p in prs],
                                       None if self_seeded else [p[2] for p in prs],
                                       None if self_seeded else [p[3] for p in prs])
    want = counts(prep=1, seed=2 if self_seeded else 0, finalize=1, planes_init=1, planes_spatial=2 * I * lanes,
                  planes_view_refine=2 * I * lanes)
    assert got == want, got
    if self_seeded:
        with pm.Engine(prm, max_rows=PLANES_SHAPE[0], max_cols=PLANES_SHAPE[1]) as e:
            ref = [e.match(p[0], p[1]) for p in prs]
    else:
        op = oracle.planes_params(**oracle.planes_kwargs_of(prm))
        ref = [oracle.planes_match(op, *p[:4]) for p in prs]
    check_maps(dl, dr, ref, f"route P, n = {n}")


def test_route_p_planes_one_view(pm, oracle, pairs):
    """left_right_check = 0: the refinement alone, one launch per iteration and lane"""
    prs = pairs[PLANES_SHAPE][:3]
    prm = pm.default_params(0, patch=7, patchmatch_iters=I, mode=pm.PM_MODE_PLANES, state_dtype=pm.PM_STATE_F32,
                            max_disp=48, left_right_check=0)
    got, dl, _ = profiled_device_call(pm, prm, PLANES_SHAPE, [p[0] for p in prs], [p[1] for p in prs],
                                      [p[2] for p in prs], None)
    assert got == counts(prep=1, finalize=1, planes_init=1, planes_spatial=2 * I * 2, planes_refine=I * 2), got
    op = oracle.planes_params(**oracle.planes_kwargs_of(prm))
    check_maps(dl, None, [(oracle.planes_match(op, p[0], p[1], p[2])[0], None) for p in prs], "route P, one view")
