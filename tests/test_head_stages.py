"""The head of a scalar Match plane by plane: prep, transposes, line planes (csrc/pm_kernels.hpp: k_prep, k_prep_bgr,
k_prep_view, k_setup; the launch plan: csrc/pm_head_plan.hpp).

Every other suite sees the head only through the disparity map that comes out many launches later.  Here every plane it
writes is read back (pm_debug_head_read, include/pm/testing.h) and compared with tests/head_ref.py bit for bit, after the
whole allocation was filled with 0x5A (pm_debug_head_poison): inside a plane's defined extent every element is the
definition's, outside it -- pitch padding, pairs the call does not have -- every byte is still 0x5A.  For a view a call
does not run, an element is the definition's or untouched.  The last test matches on poisoned planes: no result may
depend on what the padding holds.

The CPU tests at the top hold the two statements of the definition equal, pin the rounding rule of g8 and run the launch
plan's host program."""

import subprocess

import numpy as np
import pytest

import head_ref

POISON = 0x5A
POISON_OF = {1: np.uint8(0x5A), 2: np.uint16(0x5A5A), 4: np.uint32(0x5A5A5A5A)}
UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32}

# rows x cols: the smallest that reach every edge of the head
SHAPES = [(8, 8),       # the minimum
          (8, 14), (9, 15),   # ncl = 32 and 33: the column triples' tiles of 32 lines
          (64, 64),     # no pitch padding in either direction
          (65, 65),     # one past every 64-tile; nrl = 67 is no multiple of 4
          (66, 257),    # one past 256 columns; nrl = 68
          (131, 70)]    # three transpose tiles down; ncl = 88
SMALL = [(5, 9), (6, 8), (7, 64)]   # Match() on caller seeds only; the stage entry points start at 8 rows
PLAIN = ("img8", "g32", "g8", "pk16")
TRANSPOSED = ("timg8", "tg32", "tg8", "tpk16")
LINES = ("rpg", "rqk", "cpg")


def ids(shapes):
    return ["%dx%d" % s for s in shapes]


def checkerboard(rows, cols):
    """hard 0 / 255 blocks of 3 x 2 pixels: gradients far above 255, so g8 saturates"""
    yy, xx = np.mgrid[0:rows, 0:cols]
    return (((yy // 3 + xx // 2) % 2) * 255).astype(np.uint8)


_pairs = {}


def pairs_of(synth, rows, cols, n):
    """n pairs of rows x cols with seed maps: synthetic scenes, the second one the checkerboard against a scene"""
    key = (rows, cols)
    if key not in _pairs:
        ps = [synth.make_pair(40 + i, rows=rows, cols=cols, n_points=12, dilate_factor=1) for i in range(3)]
        ps[1] = dict(ps[1], left=checkerboard(rows, cols))
        _pairs[key] = ps
    return _pairs[key][:n]


_heads = {}


def head_of(oracle, left, right, key=None):
    if key is None or key not in _heads:
        plain = head_ref.plain_planes(left, right, oracle.gradient_magnitude(left), oracle.gradient_magnitude(right))
        want = head_ref.head(plain)
        if key is None:
            return want
        _heads[key] = want
    return _heads[key]


def heads_of(oracle, synth, rows, cols, n):
    return [head_of(oracle, p["left"], p["right"], (rows, cols, i)) for i, p in enumerate(pairs_of(synth, rows, cols, n))]


# ---- the definition (CPU) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, cols", SHAPES + SMALL, ids=ids(SHAPES + SMALL))
def test_the_two_statements_of_the_definition_agree(oracle, synth, rows, cols):
    for p in pairs_of(synth, rows, cols, 2):
        plain = head_ref.plain_planes(p["left"], p["right"], oracle.gradient_magnitude(p["left"]),
                                      oracle.gradient_magnitude(p["right"]))
        a, b = head_ref.head(plain, loops=True), head_ref.head(plain, loops=False)
        assert sorted(a) == sorted(PLAIN + TRANSPOSED + LINES)
        for name in a:
            assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), name
        assert a["rpg"].shape == (2, rows + 2, cols, 4) and a["rqk"].shape == (2, rows + 2, cols, 2)
        assert a["cpg"].shape == (2, cols + 18, rows, 4) and a["tg32"].shape == (4, cols + 16, rows)
        # the sentences themselves, at the corners they are about
        assert np.array_equal(a["timg8"][1, cols + 15], p["right"][:, cols - 1])
        assert a["rpg"][0, rows + 1, 0, 3] == int(p["right"][rows - 1, 0]) * 0x010101
        assert a["rqk"][1, rows - 2, 0, 0] == int(p["right"][rows - 2, cols - 1]) + int(p["right"][rows - 1, cols - 1]) * 0x01010100
        assert a["cpg"][1, cols + 17, rows - 1, 3] == int(p["left"][rows - 1, 0]) * 0x010101
        assert (a["rpg"][..., 3] >> 24 == 0).all() and (a["cpg"][..., 3] >> 24 == 0).all()
    board = head_ref.plain_planes(*[checkerboard(rows, cols)] * 2, *[oracle.gradient_magnitude(checkerboard(rows, cols))] * 2)
    assert board["g32"].max() > 255 and board["g8"].max() == 255 and board["pk16"].max() == 0xFFFF


def test_g8_rounds_halves_to_even_and_saturates():
    k = np.arange(301, dtype=np.float64)
    want = np.minimum(np.where(k % 2 == 0, k, k + 1), 255).astype(np.uint8)   # k + 0.5 goes to the even neighbour
    assert np.array_equal(head_ref.g8_rule((k + 0.5).astype(np.float32)), want)
    assert head_ref.g8_rule(np.float32(254.5)) == 254 and head_ref.g8_rule(np.float32(255.5)) == 255
    assert np.array_equal(head_ref.g8_rule(np.float32([-0.0, -0.25, -0.5, -0.75, -1.5, -300.0, -1e9])), np.zeros(7, np.uint8))
    assert np.array_equal(head_ref.g8_rule(np.float32([255.0, 255.49, 256.0, 300.7, 1e6, 3e9])), np.full(6, 255, np.uint8))
    assert np.array_equal(head_ref.g8_rule(np.float32([0.49999997, 0.50000006, 1.4999999, 2.5000002])), np.uint8([0, 1, 1, 3]))


# ---- the launch plan (CPU) -----------------------------------------------------------------------------------------------------
def test_the_setup_plan_compiles_without_hip_and_covers_every_section_exactly_once(tmp_path):
    """tests/cpp/head_plan_main.cpp: csrc/pm_head_plan.hpp through g++ (no HIP header in reach) with AddressSanitizer and UBSan,
    over the shapes above, 1 .. 3 pairs, view -1 / 0 / 1 and handles with and without line planes."""
    from cpp_build import build_host_kernel
    exe = build_host_kernel(tmp_path / "head_plan_main", "head_plan_main.cpp", compiler=("g++",),
                            flags=("-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "setup_grid: 180 plans, 0 broken\n", (r.stdout, r.stderr)


# ---- the common body of the GPU tests ----------------------------------------------------------------------------------------
def as_bits(a):
    return a.view(UNSIGNED[a.dtype.itemsize])


def check_head(e, rows, cols, wants, views_run=(0, 1), transposes_run=True, what=""):
    """The head planes of handle e (max_batch = len(wants) + 1) against the definitions `wants` of its pairs.  Returns what
    was read."""
    n = len(wants)
    s = e.debug_head_shape(rows, cols)
    assert s["max_batch"] == n + 1, "the engine of a head test has one pair more than the call"
    assert (s["pitch"], s["pitch_t"], s["nrl"], s["ncl"], s["trans_pad"]) == \
        (-(-cols // 64) * 64, -(-rows // 64) * 64, rows + 2, cols + 18, 16), s
    assert (s["plane"], s["plane_t"]) == (rows * s["pitch"], (cols + 16) * s["pitch_t"]), s
    got = e.debug_head_read(n + 1, rows, cols)
    assert sorted(got) == sorted(PLAIN + TRANSPOSED + (LINES if s["with_lines"] else ())), sorted(got)
    for name, g in got.items():
        g = as_bits(g)
        poison = POISON_OF[g.dtype.itemsize]
        want = np.full_like(g, poison)
        strict = np.ones(g.shape, bool)       # False: the element may also be untouched
        for b, w in enumerate(wants):
            d = as_bits(np.ascontiguousarray(w[name]))
            want[(b,) + tuple(slice(0, k) for k in d.shape)] = d      # the defined extent; everything else stays 0x5A
            for v in (0, 1):
                if v in views_run and (transposes_run or name in PLAIN):
                    continue
                z = [v] if name in LINES else [2 * v, 2 * v + 1]      # a view's slot, or its two planes
                strict[b, z] = False
        ok = (g == want) | (~strict & (g == poison))
        if not ok.all():
            bad = np.argwhere(~ok)
            i = tuple(int(k) for k in bad[0])
            inside = all(k < m for k, m in zip(i[1:], wants[i[0]][name].shape)) if i[0] < n else False
            raise AssertionError(f"{what}{name} {rows}x{cols}: {len(bad)} elements wrong; first at [pair, plane or slot, line, "
                                 f"element ...] = {list(i)} ({'inside' if inside else 'outside'} the defined extent): "
                                 f"{int(g[i]):#x}, want {int(want[i]):#x}")
        assert (g[n] == poison).all(), f"{what}{name}: pair {n} was written"
    return got


def engine(pm, rows, cols, n, sem=0, grow=(0, 0), **kw):
    kw.setdefault("patchmatch_iters", 0)
    prm = pm.default_params(sem, patch=3, **kw)
    return pm.Engine(prm, max_rows=max(rows + grow[0], 8), max_cols=cols + grow[1], max_batch=n + 1)   # (a plan starts at 8 rows)


def device_pairs(pairs, seeds=True):
    import torch
    dev = torch.device("cuda")

    def up(key):
        return torch.from_numpy(np.stack([p[key] for p in pairs])).to(dev).contiguous()
    L, R = up("left"), up("right")
    SL, SR = (up("seed_l"), up("seed_r")) if seeds else (None, None)
    D = torch.empty((2,) + tuple(L.shape), dtype=torch.float32, device=dev)
    return L, R, SL, SR, D


def match_device(e, rows, cols, pairs, seeds=True):
    L, R, SL, SR, D = device_pairs(pairs, seeds)
    e.match_device(len(pairs), L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr() if seeds else None,
                   SR.data_ptr() if seeds else None, D[0].data_ptr(), D[1].data_ptr() if e.params.left_right_check else None)
    e.synchronize()


# ---- the routes of pm_match_device -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rows, cols", SHAPES + SMALL, ids=ids(SHAPES + SMALL))
def test_one_stream_route(pm, oracle, synth, rows, cols):
    """left_right_check = 0: one head for all four planes of both pairs on the handle's stream"""
    n = 2
    assert pm.match_plan(pm.default_params(0, left_right_check=0), n, True, True)["route"] == pm.ROUTE_ONE_STREAM
    with engine(pm, rows, cols, n, left_right_check=0) as e:
        e.debug_head_poison(POISON)
        match_device(e, rows, cols, pairs_of(synth, rows, cols, n))
        check_head(e, rows, cols, heads_of(oracle, synth, rows, cols, n), views_run=(0,))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("rows, cols", SHAPES + SMALL, ids=ids(SHAPES + SMALL))
def test_view_heads_on_two_streams(pm, oracle, synth, rows, cols, n):
    """left_right_check = 1, up to two pairs: each view's head on its own stream, at the same time -- on a handle whose
    plan is larger than the images, so that the planes of a pair do not end where the allocation's do"""
    assert pm.match_plan(pm.default_params(0), n, True, True)["route"] == pm.ROUTE_VIEW_HEADS
    with engine(pm, rows, cols, n, grow=(5, 67)) as e:
        e.debug_head_poison(POISON)
        match_device(e, rows, cols, pairs_of(synth, rows, cols, n))
        check_head(e, rows, cols, heads_of(oracle, synth, rows, cols, n))


@pytest.mark.gpu
@pytest.mark.parametrize("rows, cols", SHAPES + SMALL, ids=ids(SHAPES + SMALL))
def test_chunks_with_a_last_chunk_of_one_pair(pm, oracle, synth, rows, cols):
    n = 3
    assert pm.match_plan(pm.default_params(0), n, True, True)["route"] == pm.ROUTE_CHUNKS
    with engine(pm, rows, cols, n) as e:
        e.debug_head_poison(POISON)
        match_device(e, rows, cols, pairs_of(synth, rows, cols, n))
        check_head(e, rows, cols, heads_of(oracle, synth, rows, cols, n))


@pytest.mark.gpu
@pytest.mark.parametrize("lr", [0, 1])
@pytest.mark.parametrize("rows, cols", SHAPES, ids=ids(SHAPES))
def test_the_seed_copy_riding_in_prep_changes_no_image_plane(pm, oracle, synth, rows, cols, lr):
    """with caller seeds the per-view route copies them inside k_prep; without, the planes must be the same"""
    n = 2
    got = []
    for seeds in (True, False):
        with engine(pm, rows, cols, n, left_right_check=lr) as e:
            e.debug_head_poison(POISON)
            match_device(e, rows, cols, pairs_of(synth, rows, cols, n), seeds=seeds)
            got.append(check_head(e, rows, cols, heads_of(oracle, synth, rows, cols, n), views_run=(0, 1) if lr else (0,),
                                  what="seeds " if seeds else "no seeds "))
    for name in got[0]:
        assert np.array_equal(as_bits(got[0][name]), as_bits(got[1][name])), name


# ---- the BGR entry -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rows, cols", [(65, 65), (66, 257)], ids=ids([(65, 65), (66, 257)]))
def test_bgr_entry_writes_the_planes_of_the_stereo_ready_gray(pm, oracle, synth, rows, cols):
    """pm_match_bgr_device: k_prep_bgr computes the enhanced gray in its 66 x 10 ring.  img8 against pm_stereo_ready's
    gray image of the same BGR image, everything else from the definition on that gray image."""
    import torch
    n = 2
    dev = torch.device("cuda")
    pairs = pairs_of(synth, rows, cols, n)
    bgr = [[synth.to_bgr(p[k], 7 + 2 * i + j) for j, k in enumerate(("left", "right"))] for i, p in enumerate(pairs)]
    BL = torch.from_numpy(np.stack([b[0] for b in bgr])).to(dev).contiguous()
    BR = torch.from_numpy(np.stack([b[1] for b in bgr])).to(dev).contiguous()
    D = torch.empty((2, n, rows, cols), dtype=torch.float32, device=dev)
    J = torch.empty((rows, cols, 3), dtype=torch.float32, device=dev)
    G = torch.empty((n, 2, rows, cols), dtype=torch.uint8, device=dev)
    with engine(pm, rows, cols, n) as e:
        for i in range(n):
            for j, B in enumerate((BL, BR)):
                e.stereo_ready(B[i].data_ptr(), rows, cols, J.data_ptr(), G[i, j].data_ptr())
        e.synchronize()
        e.debug_head_poison(POISON)
        e.match_bgr_device(n, BL.data_ptr(), BR.data_ptr(), rows, cols, None, None, D[0].data_ptr(), D[1].data_ptr())
        e.synchronize()
        gray = G.cpu().numpy()
        assert all(len(np.unique(g)) > 2 for g in gray.reshape(-1, rows, cols))
        check_head(e, rows, cols, [head_of(oracle, gray[i, 0], gray[i, 1]) for i in range(n)])


# ---- the view entry: caller gradients ------------------------------------------------------------------------------------------
TIES = np.float32([0.5, 1.5, 2.5, 3.5, 126.5, 127.5, 254.5, 255.5, 255.51, 256.0, 300.7, 1e6, -0.0, -0.25, -0.5, -0.75, -3.0,
                   0.0, 17.0, 254.49998, 254.50002])


@pytest.mark.gpu
@pytest.mark.parametrize("rows, cols", SHAPES, ids=ids(SHAPES))
def test_view_entry_takes_the_callers_gradients_as_given(pm, oracle, synth, rows, cols):
    """pm_match_view_device with a row step wider than a row: g32 comes back bit for bit, g8 rounds halves to even.  The
    call writes planes 0 and 1; planes 2 and 3 stay poisoned, and what k_setup derives for view 1 is derived from that."""
    import torch
    dev = torch.device("cuda")
    p = pairs_of(synth, rows, cols, 1)[0]
    padc = cols + 9
    rng = np.random.default_rng(rows * 1000 + cols)
    gl, gr = (TIES[(np.arange(rows * cols) * step + off) % len(TIES)].reshape(rows, cols) for step, off in ((1, 0), (5, 3)))
    gr = np.where(rng.random((rows, cols)) < 0.3, rng.uniform(0, 400, (rows, cols)).astype(np.float32), gr)

    def padded(a):
        buf = torch.full((rows, padc), -7.0, dtype=torch.float32, device=dev)
        buf[:, :cols] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        return buf
    IL, IR, GL, GR, D = padded(p["left"]), padded(p["right"]), padded(gl), padded(gr), padded(p["seed_l"])
    others = {"img8": 0x5A, "g8": 0x5A, "pk16": 0x5A5A, "g32": np.uint32(0x5A5A5A5A).view(np.float32)}
    want = head_ref.head(head_ref.plain_planes_of_view(p["left"].astype(np.float32), p["right"].astype(np.float32), gl, gr, others))
    with engine(pm, rows, cols, 1, left_right_check=0) as e:
        e.debug_head_poison(POISON)
        e.match_view_device(IL.data_ptr(), IR.data_ptr(), GL.data_ptr(), GR.data_ptr(), rows, cols, padc * 4, D.data_ptr(),
                            padc * 4)
        e.synchronize()
        got = check_head(e, rows, cols, [want], views_run=(0,))
    assert np.array_equal(as_bits(got["g32"][0, 0, :, :cols]), head_ref.bits(gl))
    assert np.array_equal(got["g8"][0, 1, :, :cols], head_ref.g8_rule(gr))
    assert {0, 2, 4, 128, 254, 255} <= set(np.unique(got["g8"][0, 0, :, :cols]).tolist())


# ---- a stage entry point, and the handles without line planes ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rows, cols", SHAPES, ids=ids(SHAPES))
def test_stage_entry_point_prepares_the_same_head(pm, oracle, synth, rows, cols):
    p = pairs_of(synth, rows, cols, 2)[1]
    with engine(pm, rows, cols, 1) as e:
        e.debug_head_poison(POISON)
        e.debug_noise_cost(p["left"], p["right"], p["seed_l"], 3, 3)
        check_head(e, rows, cols, [head_of(oracle, p["left"], p["right"], (rows, cols, 1))])
        for shape in SMALL:
            with pytest.raises(pm.PmError) as err:
                e.debug_noise_cost(p["left"][:shape[0]], p["right"][:shape[0]], p["seed_l"][:shape[0]], 3, 3)
            assert err.value.status == pm.PM_ERR_INVALID_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sem_gpu", "planes", "planes_stage"])
@pytest.mark.parametrize("rows, cols", SHAPES, ids=ids(SHAPES))
def test_handles_without_line_planes(pm, oracle, synth, rows, cols, kind):
    """PM_SEM_GPU and PM_MODE_PLANES: with_lines = 0.  A PM_SEM_GPU Match and every stage entry point transpose; a plane-mode
    Match runs the prep kernel alone, so there the transposes stay untouched."""
    n = 2
    pairs, wants = pairs_of(synth, rows, cols, n), heads_of(oracle, synth, rows, cols, n)
    if kind == "sem_gpu":
        e = engine(pm, rows, cols, n, sem=1)
    else:
        n = n if kind == "planes" else 1
        e = engine(pm, rows, cols, n, mode=pm.PM_MODE_PLANES, max_disp=16, patchmatch_iters=1)
    with e:
        assert e.debug_head_shape(rows, cols)["with_lines"] == 0
        e.debug_head_poison(POISON)
        if kind == "planes_stage":
            e.gradient_magnitude(pairs[1]["left"])
            wants = [head_of(oracle, pairs[1]["left"], pairs[1]["left"])]
        else:
            match_device(e, rows, cols, pairs, seeds=kind == "sem_gpu")
        got = check_head(e, rows, cols, wants, transposes_run=kind != "planes")
        assert sorted(got) == sorted(PLAIN + TRANSPOSED)
        if kind == "planes":
            assert all((as_bits(got[name]) == POISON_OF[got[name].dtype.itemsize]).all() for name in TRANSPOSED)
        for name in LINES:
            with pytest.raises(pm.PmError) as err:
                e.debug_head_read(1, rows, cols, planes=[name])
            assert err.value.status == pm.PM_ERR_INVALID_ARG


# ---- what the hooks refuse ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hooks_refuse_captures_pairs_in_flight_bad_bytes_and_sizes(pm, synth):
    rows, cols = 16, 24
    p = pairs_of(synth, rows, cols, 1)[0]

    def status(call, *a, **kw):
        with pytest.raises(pm.PmError) as err:
            call(*a, **kw)
        return err.value.status
    with engine(pm, rows, cols, 1) as e:
        for byte in (255, 256, -1):
            assert status(e.debug_head_poison, byte) == pm.PM_ERR_INVALID_ARG
        e.debug_head_poison(0)
        e.debug_head_poison(254)
        for r, c, k in ((4, 24, 1), (16, 7, 1), (17, 24, 1), (16, 25, 1), (0, 0, 1), (16, 24, 0), (16, 24, 3)):
            assert status(e.debug_head_read, k, r, c) == pm.PM_ERR_INVALID_ARG, (r, c, k)
        assert status(e.debug_head_shape, 4, 24) == pm.PM_ERR_INVALID_ARG
        assert e.debug_head_shape(5, 8)["nrl"] == 7            # Match()'s own minimum on caller seeds
        assert e.debug_head_read(1, 16, 24, planes=[]) == {}
        L, R, SL, SR, D = device_pairs([p])

        def run():
            e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), D[0].data_ptr(), D[1].data_ptr())
        run()                # once outside: the noise table and the events a capture cannot create
        e.synchronize()
        e.capture_begin()
        try:
            busy = [status(e.debug_head_poison, POISON), status(e.debug_head_read, 1, rows, cols), status(e.debug_head_shape, rows, cols)]
            run()
        finally:
            e.capture_end()      # (a refused hook leaves the capture open and usable)
        assert busy == [pm.PM_ERR_BUSY] * 3
        e.replay()
        e.synchronize()
        e.submit(p["left"], p["right"], p["seed_l"], p["seed_r"])
        busy = [status(e.debug_head_poison, POISON), status(e.debug_head_read, 1, rows, cols), status(e.debug_head_shape, rows, cols)]
        e.collect()
        assert busy == [pm.PM_ERR_BUSY] * 3
        e.debug_head_poison(POISON)
        assert all((as_bits(a) == POISON_OF[a.dtype.itemsize]).all() for a in e.debug_head_read(2, rows, cols).values())
    with engine(pm, rows, cols, 1, sparse_init=1) as e:
        assert status(e.debug_head_shape, 5, 8) == pm.PM_ERR_INVALID_ARG   # a self-seeding handle starts at 8 rows


# ---- no result depends on what the padding holds ----------------------------------------------------------------------------------
PADDING_CASES = [(37, 83, 5), (37, 83, 11), (70, 131, 5), (70, 131, 11)]
_padding = {}


def padding_case(oracle, synth, rows, cols, patch):
    key = (rows, cols, patch)
    if key not in _padding:
        p = synth.make_pair(61, rows=rows, cols=cols, n_points=30, dilate_factor=2)
        want = oracle.match(oracle.default_params(0, patch=patch, n_iters=2, nthreads=4), p["left"], p["right"], p["seed_l"],
                            p["seed_r"])
        _padding[key] = (p, want)
    return _padding[key]


@pytest.mark.parametrize("rows, cols, patch", PADDING_CASES)
def test_the_oracles_maps_of_the_padding_cases_are_not_empty(oracle, synth, rows, cols, patch):
    _, (wl, wr) = padding_case(oracle, synth, rows, cols, patch)
    assert (wl > 0).mean() > 0.2 and (wr > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("rows, cols, patch", PADDING_CASES)
def test_a_match_does_not_depend_on_what_the_padding_holds(pm, oracle, synth, rows, cols, patch):
    """The sweeps read row padding behind cols / rows (with weight 0, or by lanes out of reach).  After a poison every such
    element holds 1.5e16 (0x5A bytes) instead of the zeros of a fresh handle; both must give the oracle's maps."""
    p, (wl, wr) = padding_case(oracle, synth, rows, cols, patch)
    assert (wl > 0).mean() > 0.2
    for poisoned in (True, False):
        with pm.Engine(pm.default_params(0, patch=patch, patchmatch_iters=2), max_rows=rows, max_cols=cols, max_batch=1) as e:
            if poisoned:
                e.debug_head_poison(POISON)
            dl, dr = e.match(p["left"], p["right"], p["seed_l"], p["seed_r"])
        what = "poisoned" if poisoned else "fresh"
        assert np.array_equal(dl.view(np.uint32), wl.view(np.uint32)), f"{what}, left: {int((dl != wl).sum())} pixels differ"
        assert np.array_equal(dr.view(np.uint32), wr.view(np.uint32)), f"{what}, right: {int((dr != wr).sum())} pixels differ"
