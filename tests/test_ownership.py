"""Everything a handle or a tiled plan takes from the runtime has one owner -- device allocations csrc/pm_devbuf.hpp;
events, streams, page-locked host memory and instantiated graphs csrc/pm_hipres.hpp: the process-wide counters of what
is live (include/pm/testing.h) return to where they were after pm_destroy / pm_tiled_destroy -- also after a pm_create
that failed half way -- and every scratch buffer that grows on demand gives the same bits small -> large -> small."""
import collections
import ctypes as C

import numpy as np
import pytest

import guided_ref as G
import oracle_lib as O
import rectify_ref as RR
from conftest import assert_same, small_pair
from test_enhance import color_image
from test_guided import range_scene
from test_rectify import radtan_view, rot


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


Live = collections.namedtuple("Live", "device_allocations device_bytes events streams host_buffers host_bytes graph_execs")


def _live(pm):
    lib = pm.load()
    return Live(*(getattr(lib, "pm_debug_live_" + name)() for name in Live._fields))


# the seeder's template, search range and cornerSubPix window cut down to what a 16x24 image holds
SMALL_SEEDER = dict(templ_cols=7, templ_rows=7, max_disp=16, max_features_per_frame=50, min_distance_btw_features=3,
                    subpix_winsize=2)
PARAM_SETS = {
    "scalar_cpu_run_engine": lambda pm: (pm.default_params(pm.PM_SEM_CPU, patch=5, patchmatch_iters=2), True),
    "scalar_self_seeded_subpix": lambda pm: (pm.default_params(pm.PM_SEM_GPU, patch=3, patchmatch_iters=2, sparse_init=1,
                                                               subpixel_corners=1, **SMALL_SEEDER), True),
    "planes_f16": lambda pm: (pm.default_params(pm.PM_SEM_CPU, patch=5, patchmatch_iters=1, mode=pm.PM_MODE_PLANES,
                                                state_dtype=pm.PM_STATE_F16, max_disp=16), False),
}


def _exercise_every_lazy_family(pm, synth, e, seeded, scalar):
    """One call of every family that allocates, or creates events, a graph or page-locked memory, on first use, at 16x24
    on a 32x48 plan of two pairs.  Returns what has to outlive the handle."""
    import torch
    rows, cols = 16, 24
    l, r, sl, sr, _ = small_pair(synth, 3, rows, cols, n_points=6, dilate_factor=1)
    seeds = (sl, sr) if seeded else ()
    e.match(l, r, *seeds)                                                              # pm_match_u8: left_out / right_out
    e.match_batch([l, l], [r, r], *([s, s] for s in seeds))                            # the ring-slot and view events
    e.submit(l, r, *seeds)
    e.collect()
    e.profile_enable(True)                                                             # the pool of timed event pairs
    e.match(l, r, *seeds)
    e.profile_read()
    e.profile_enable(False)
    kept = e.host_alloc((rows, cols), np.float32, owned=True)  # never freed: pm_destroy gives it back (not touched after)
    mine = np.empty((rows, cols), np.float32)                  # never unregistered either; the memory stays numpy's
    e.host_register(mine)
    del kept
    bgr8 = np.stack([color_image(rows, cols, 5 + i) for i in range(4)])
    B = _dev(bgr8)
    J = torch.empty((rows, cols, 3), device="cuda")
    gray = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
    e.stereo_ready(B.data_ptr(), rows, cols, J.data_ptr(), gray.data_ptr())
    D = [torch.empty((2, rows, cols), device="cuda") for _ in range(2)]
    e.match_bgr_device(2, B[:2].data_ptr(), B[2:].data_ptr(), rows, cols, None, None, D[0].data_ptr(), D[1].data_ptr())
    guide, src = range_scene(rows, cols, 7)
    d_g, d_p = _dev(guide), _dev(src)
    d_o = torch.empty_like(d_p)
    e.fast_guided_filter(d_g.data_ptr(), d_p.data_ptr(), rows, cols, 3, 4, 0.01, 2, 1.0, d_o.data_ptr())
    e.gather_pixels(d_p.data_ptr(), rows, cols, 3, xy=[[0, 0], [23, 15], [5, 7]])
    ident = RR.identity_view(30.0, 30.0, cols / 2, rows / 2)
    L, R = _dev(l), _dev(r)
    e.match_raw_device(1, ident, ident, L.data_ptr(), R.data_ptr(), rows, cols, 0, rows, cols, None, None,
                       D[0].data_ptr(), D[1].data_ptr())
    mask = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
    e.foreground_texture_mask(L.data_ptr(), rows, cols, 4, 10.0, 2, mask.data_ptr())
    SL, SR = _dev(sl), _dev(sr)
    if scalar:  # one view on a foreign stream: ext_fork / ext_join
        IL, IR, GL, GR = (_dev(a.astype(np.float32)) for a in (l, r, e.gradient_magnitude(l), e.gradient_magnitude(r)))
        DV = SL.clone()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        e.match_view_device(IL.data_ptr(), IR.data_ptr(), GL.data_ptr(), GR.data_ptr(), rows, cols, 0, DV.data_ptr(), 0,
                            stream=side.cuda_stream)
        side.synchronize()
    if scalar and seeded:  # a captured Match() on caller seeds (what tests/test_gpu_parity.py captures), run once before
        run = lambda: e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(),
                                     D[0].data_ptr(), D[1].data_ptr())
        run()
        e.synchronize()
        e.capture_begin()
        run()
        e.capture_end()
        e.replay()
        e.synchronize()
    if scalar:  # the top band of a taller image (scalar mode only: the plane mode has no tile API)
        e.tile_begin(pm.PmTile(rows + 100, 0, 0, rows - 5), L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(),
                     SR.data_ptr())
        e.tile_snapshot()
    e.synchronize()
    return mine


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PARAM_SETS))
def test_create_use_destroy_returns_every_byte(pm, synth, name):
    params, scalar = PARAM_SETS[name](pm)
    seeded = not params.sparse_init
    before = _live(pm)
    for cycle in range(5):
        with pm.Engine(params, max_rows=32, max_cols=48, max_batch=2) as e:
            created = _live(pm)
            assert created.device_allocations > before.device_allocations and created.device_bytes > before.device_bytes
            assert created.streams > before.streams, "the handle's streams are counted"
            assert created.host_buffers > before.host_buffers and created.host_bytes > before.host_bytes, "the staging slab"
            registered = _exercise_every_lazy_family(pm, synth, e, seeded, scalar)
            used = _live(pm)
            assert used.device_allocations > created.device_allocations and used.device_bytes > created.device_bytes, \
                "the lazily allocated buffers are counted too"
            assert used.events > created.events, "the lazily created events are counted"
            assert used.host_buffers == created.host_buffers + 2 and used.host_bytes == created.host_bytes + 2 * registered.nbytes
            assert used.graph_execs == created.graph_execs + (1 if scalar and seeded else 0)
        assert _live(pm) == before, "cycle %d: %r live, %r before the create" % (cycle, _live(pm), before)
        registered[:] = 1.0  # the registered array was only unlocked: it is still numpy's memory


@pytest.mark.gpu
def test_create_that_fails_half_way_leaks_nothing(pm):
    """validate_params accepts a 15x15 window with max_disp 1024; planes_alloc refuses its LDS need (pm_planes.hpp:
    pl_lds_bytes -- more than 2 x 22 rows x 1200 columns of 4-byte pairs) after the scalar planes, the state planes and the
    seeder's scratch were allocated."""
    lib = pm.load()
    params = pm.default_params(pm.PM_SEM_CPU, patch=15, mode=pm.PM_MODE_PLANES, max_disp=1024)
    before = _live(pm)
    h = C.c_void_p()
    rc = lib.pm_create(C.byref(params), 0, 16, 24, 1, C.byref(h))
    assert rc == pm.PM_ERR_INVALID_ARG and h
    text = lib.pm_last_error(h).decode()
    assert "KB of LDS per tile" in text and "max_disp 1024" in text, text
    held = _live(pm)
    assert held.device_allocations > before.device_allocations and held.device_bytes > before.device_bytes, \
        "the create got as far as allocating"
    assert held.streams > before.streams, "... with its streams live"
    lib.pm_destroy(h)
    assert _live(pm) == before


# ---- every grower, small -> large -> small on one handle ----------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(pm.PM_SEM_CPU, patch=5, patchmatch_iters=2), max_rows=32, max_cols=48,
                   max_batch=2) as e:
        yield e


@pytest.mark.gpu
def test_gaussian_scratch_and_taps_regrow(engine):
    import torch

    def blur(rows, cols, ksize):
        img = np.random.default_rng(rows + ksize).uniform(0, 1, (rows, cols, 3)).astype(np.float32)
        d_in = _dev(img)
        d_out = torch.empty_like(d_in)
        engine.gaussian_blur(d_in.data_ptr(), rows, cols, 3, ksize, ksize / 4.0, d_out.data_ptr())
        engine.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), O.gaussian_blur(img, ksize, ksize / 4.0)), (rows, cols, ksize)

    for rows, cols in ((16, 24), (40, 64), (16, 24)):
        blur(rows, cols, 9)
    for ksize in (5, 21, 5):
        blur(16, 24, ksize)


@pytest.mark.gpu
def test_bgr_match_scratch_regrows(engine):
    """n = 1, 2, 1: both the blurred illuminants and the min / max words grow; the reference is the one of
    test_enhance.py, pm_stereo_ready x 2 + pm_match_device."""
    import torch
    rows, cols = 32, 48
    px = rows * cols
    BL, BR = (_dev(np.stack([color_image(rows, cols, s + i) for i in range(2)])) for s in (11, 17))
    GL = torch.empty((2, rows, cols), dtype=torch.uint8, device="cuda")
    GR = torch.empty_like(GL)
    for i in range(2):
        engine.stereo_ready(BL.data_ptr() + 3 * px * i, rows, cols, None, GL.data_ptr() + px * i)
        engine.stereo_ready(BR.data_ptr() + 3 * px * i, rows, cols, None, GR.data_ptr() + px * i)
    want = [torch.empty((2, rows, cols), device="cuda") for _ in range(2)]
    engine.match_device(2, GL.data_ptr(), GR.data_ptr(), rows, cols, None, None, want[0].data_ptr(), want[1].data_ptr())
    for n in (1, 2, 1):
        got = [torch.full((2, rows, cols), -7.0, device="cuda") for _ in range(2)]
        engine.match_bgr_device(n, BL.data_ptr(), BR.data_ptr(), rows, cols, None, None, got[0].data_ptr(),
                                got[1].data_ptr())
        engine.synchronize()
        assert torch.equal(got[0][:n], want[0][:n]) and torch.equal(got[1][:n], want[1][:n]), n


@pytest.mark.gpu
def test_guided_filter_scratch_regrows(engine):
    import torch
    for rows, cols in ((24, 32), (48, 64), (24, 32)):
        guide, src = range_scene(rows, cols, rows)
        d_g, d_p = _dev(guide), _dev(src)
        d_o = torch.empty_like(d_p)
        engine.fast_guided_filter(d_g.data_ptr(), d_p.data_ptr(), rows, cols, 3, 4, 0.01, 2, 1.0, d_o.data_ptr())
        engine.synchronize()
        assert np.array_equal(d_o.cpu().numpy(), G.fast_guided_filter(guide, src, 4, 0.01, 2)), (rows, cols)


@pytest.mark.gpu
def test_gather_scratch_regrows(engine):
    rows, cols = 32, 48
    _, bgr = range_scene(rows, cols, 3)
    d_b = _dev(bgr)
    rng = np.random.default_rng(4)
    for n in (3, 300, 3):
        xy = np.stack([rng.integers(0, cols, n), rng.integers(0, rows, n)], axis=1)
        assert np.array_equal(engine.gather_pixels(d_b.data_ptr(), rows, cols, 3, xy=xy), bgr[xy[:, 1], xy[:, 0]]), n


@pytest.mark.gpu
def test_rectified_pair_scratch_regrows(engine, synth):
    """The reference is the one of test_rectify.py: pm_rectify_u8 x 2 + pm_match_device."""
    import torch
    for rows, cols in ((16, 24), (32, 48)):
        l, r, sl, sr, _ = small_pair(synth, 5, rows, cols, n_points=8, dilate_factor=1)
        vl = radtan_view(rows, cols, rows, cols, zoom=1.0)
        vr = radtan_view(rows, cols, rows, cols, R=rot(0, 0.7) @ rot(1, -1.5), zoom=1.0)
        L, R, SL, SR = _dev(l), _dev(r), _dev(sl), _dev(sr)
        RL, RRt = torch.empty_like(L), torch.empty_like(R)
        out = [torch.full((rows, cols), -7.0, device="cuda") for _ in range(4)]
        engine.rectify_u8(vl, L.data_ptr(), 1, rows, cols, 0, rows, cols, 0, RL.data_ptr())
        engine.rectify_u8(vr, R.data_ptr(), 1, rows, cols, 0, rows, cols, 0, RRt.data_ptr())
        engine.match_device(1, RL.data_ptr(), RRt.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), out[0].data_ptr(),
                            out[1].data_ptr())
        engine.match_raw_device(1, vl, vr, L.data_ptr(), R.data_ptr(), rows, cols, 0, rows, cols, SL.data_ptr(),
                                SR.data_ptr(), out[2].data_ptr(), out[3].data_ptr())
        engine.synchronize()
        assert np.array_equal(RL.cpu().numpy(), RR.rectify(l, vl, rows, cols)[0])
        assert torch.equal(out[2], out[0]) and torch.equal(out[3], out[1]) and not bool((out[0] == -7.0).all())


@pytest.mark.gpu
def test_noise_table_is_rebuilt_for_each_size(engine, oracle, synth):
    for rows, cols in ((16, 24), (32, 48), (16, 24)):
        l, r, sl, sr, _ = small_pair(synth, 6, rows, cols, n_points=8, dilate_factor=1)
        dl, dr = engine.match(l, r, sl, sr)
        el, er = oracle.match(oracle.default_params(0, patch=5, n_iters=2, nthreads=4), l, r, sl, sr)
        assert_same(dl, el, "left %dx%d" % (cols, rows))
        assert_same(dr, er, "right %dx%d" % (cols, rows))


@pytest.fixture(scope="module")
def two_band_pair(oracle, synth):
    """A 64x48 pair for two bands and its untiled maps: (left, right, seed_l, seed_r, want_l, want_r)."""
    l, r, sl, sr, _ = small_pair(synth, 8, 64, 48, n_points=12, dilate_factor=2)
    el, er = oracle.match(oracle.default_params(0, patch=5, n_iters=2, nthreads=4), l, r, sl, sr)
    return l, r, sl, sr, el, er


@pytest.mark.gpu
def test_noise_table_of_a_band_grows_past_the_plan(pm, two_band_pair):
    """Two bands of a 64x48 image: each handle's plan holds its band only, its noise table the whole image's rows."""
    import tiled
    l, r, sl, sr, el, er = two_band_pair
    rows, cols = l.shape
    params = pm.default_params(0, patch=5, patchmatch_iters=2)
    assert tiled.band_of(0, 2, rows, tiled.halo_rows(params))[3] < rows
    dl, dr, _ = tiled.match_tiled_local(params, l, r, sl, sr, 2, pipelined=True)
    assert_same(dl, el, "tiled vs oracle (left)")
    assert_same(dr, er, "tiled vs oracle (right)")


@pytest.mark.gpu
@pytest.mark.parametrize("logical", [None, [0, 1]])
def test_a_tiled_plan_returns_everything(pm, two_band_pair, logical):
    """pm_tiled_create / pm_tiled_match_u8 / pm_tiled_destroy over two band handles: a band's twelve buffers and six
    events (seven with the probe event of a logical-device plan) are counted while the plan lives and gone after it."""
    l, r, sl, sr, el, er = two_band_pair
    rows, cols = l.shape
    params = pm.default_params(0, patch=5, patchmatch_iters=2)
    n = 2
    before = _live(pm)
    band_rows = pm.load().pm_tiled_band_rows(C.byref(params), rows, n)
    handles = [pm.Engine(params, max_rows=band_rows, max_cols=cols) for _ in range(n)]
    alone = _live(pm)  # what the band handles hold by themselves
    for h in handles:
        h.close()
    assert _live(pm) == before
    with pm.TiledEngine(params, rows, cols, n, logical_devices=logical) as t:
        planned = _live(pm)
        assert planned.device_allocations == alone.device_allocations + 12 * n and planned.device_bytes > alone.device_bytes
        assert planned.events == alone.events + (7 if logical else 6) * n
        assert planned.streams == alone.streams and planned.host_buffers == alone.host_buffers
        dl, dr, _ = t.match(l, r, sl, sr)
        assert_same(dl, el, "tiled vs oracle (left)")
        assert_same(dr, er, "tiled vs oracle (right)")
        assert _live(pm).device_allocations >= planned.device_allocations and _live(pm).events >= planned.events
    assert _live(pm) == before
