"""The speckle filter between Match() and the cloud / normals stages: connected regions of similar disparity, small ones set
to 0 (include/pm/imaging.h: pm_filter_speckles).

CPU tests pin the definition (tests/speckle_ref.py) against an independent construction (scipy's connected_components on
the explicit edge list), against a flood fill and against hand-written answers, and run the kernels' own per-thread code
(csrc/pm_speckle_body.hpp) on the host under ASan / UBSan.  GPU tests hold the four launches to the definition with
tolerance 0 -- labels, sizes, output bits and the removed count -- with guard bands around every output."""
import ctypes as C
import functools
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import speckle_ref as SR
from conftest import ROOT
from cpp_build import CSRC, SANITIZE, build_host_kernel

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_cloud as FC  # noqa: E402
import fuzz_normals as FN  # noqa: E402
import fuzz_speckle as FS  # noqa: E402  (check_speckles: the device-against-definition comparison; pattern: the maps)

gpu = pytest.mark.gpu
SMALL_SHAPES = ("1x1", "1x(T+1)", "(R+1)x1", "RxT", "(R+1)x(T+1)", "(2R+3)x(2T+5)")


# ---- 1. the definition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.3, 0.6, 0.95])
def test_definition_against_scipy_connected_components(density):
    """An independent construction: the explicit list of joined 4-neighbour pairs as a sparse graph, scipy's components of
    it, each mapped to its smallest pixel index.  Sizes, labels and the removed set agree; so does the flood fill."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    rows, cols, max_diff, max_size = 40, 70, 1.0, 20
    disp = FN.run_map(np.random.default_rng(int(density * 100)), rows, cols, valid=density, special=0.05)
    got = SR.filter_speckles(disp, max_diff, max_size)
    d64 = disp.astype(np.float64)
    valid = disp > 0
    pairs = []
    with np.errstate(invalid="ignore"):
        for y in range(rows):
            for x in range(cols):
                for qy, qx in ((y, x + 1), (y + 1, x)):
                    if qy < rows and qx < cols and valid[y, x] and valid[qy, qx] and abs(d64[y, x] - d64[qy, qx]) <= max_diff:
                        pairs.append((y * cols + x, qy * cols + qx))
    pairs = np.array(pairs, np.int64).reshape(-1, 2)
    n = rows * cols
    graph = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    smallest = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    labels = np.where(valid.ravel(), smallest[comp], -1).reshape(rows, cols)
    sizes = np.where(valid.ravel(), np.bincount(comp)[comp], 0).reshape(rows, cols)
    assert np.array_equal(got["labels"], labels) and np.array_equal(got["sizes"], sizes)
    gone = valid & (sizes <= max_size)
    assert np.array_equal(got["out"] == 0, gone | (disp == 0)) and got["removed"] == int(gone.sum()) > 0
    assert np.array_equal(FC.bits(got["out"])[~gone], FC.bits(disp)[~gone])
    assert density < 0.5 or (sizes > max_size).any()
    fill = SR.filter_speckles(disp, max_diff, max_size, components=SR.components_bfs)
    assert all(np.array_equal(FC.bits(got[k]), FC.bits(fill[k])) for k in ("out", "labels", "sizes"))


def test_known_answers():
    # a 3x3 map with a centre hole: one ring of 8 whose smallest index is 0
    d = np.full((3, 3), 5.0, np.float32)
    d[1, 1] = 0.0
    r = SR.filter_speckles(d, 1.0, 7)
    assert r["labels"].tolist() == [[0, 0, 0], [0, -1, 0], [0, 0, 0]] and r["sizes"].tolist() == [[8, 8, 8], [8, 0, 8], [8, 8, 8]]
    assert r["removed"] == 0 and np.array_equal(FC.bits(r["out"]), FC.bits(d))
    r = SR.filter_speckles(d, 1.0, 8)
    assert r["removed"] == 8 and (r["out"] == 0).all() and not np.signbit(r["out"]).any()
    # two touching regions whose difference is exactly max_diff: joined; with the next float above: not joined
    d = np.array([[8.0, 8.0, 8.5, 8.5]], np.float32)  # 0.5 and 8.5 - 8 are exact in binary32
    assert SR.filter_speckles(d, 0.5, 0)["labels"].tolist() == [[0, 0, 0, 0]]
    assert SR.filter_speckles(d, 0.5, 0)["sizes"].tolist() == [[4, 4, 4, 4]]
    d[0, 2:] = np.nextafter(np.float32(8.5), np.float32(9))
    r = SR.filter_speckles(d, 0.5, 2)
    assert r["labels"].tolist() == [[0, 0, 2, 2]] and r["sizes"].tolist() == [[2, 2, 2, 2]] and r["removed"] == 4
    # +inf is valid and a component of its own, also next to +inf; NaN, -0.0 and negatives are invalid and keep their bits
    d = np.array([[np.inf, np.inf, 3.0, np.nan, 3.0, -0.0, 3.0, -2.0, 3.0]], np.float32)
    r = SR.filter_speckles(d, 1e30, 1)
    assert r["labels"].tolist() == [[0, 1, 2, -1, 4, -1, 6, -1, 8]] and r["sizes"].tolist() == [[1, 1, 1, 0, 1, 0, 1, 0, 1]]
    assert r["removed"] == 6
    want = np.array([[0.0, 0.0, 0.0, np.nan, 0.0, -0.0, 0.0, -2.0, 0.0]], np.float32)
    assert np.array_equal(FC.bits(r["out"]), FC.bits(want))
    # a slow ramp is one component; max_size = 0 removes nothing and still labels
    d = (1.0 + 0.5 * np.arange(12, dtype=np.float32)).reshape(1, 12)
    r = SR.filter_speckles(d, 0.5, 0)
    assert (r["labels"] == 0).all() and (r["sizes"] == 12).all() and r["removed"] == 0 and np.array_equal(r["out"], d)
    # no diagonals
    d = np.array([[4.0, 0.0], [0.0, 4.0]], np.float32)
    assert SR.filter_speckles(d, 1.0, 0)["labels"].tolist() == [[0, -1], [-1, 3]]


def test_patterns_are_what_they_claim():
    """The maps of tools/fuzz_speckle.py at the largest small shape: the component counts each is built to have."""
    T, R = 64, 16
    rows, cols = 2 * R + 3, 2 * T + 5
    rng = np.random.default_rng(1)
    count = lambda r: int((r["labels"].ravel() == np.arange(rows * cols)).sum())
    for name, components in (("constant", 1), ("serpentine", 1), ("comb", 1), ("spiral", 1), ("two_combs", 2)):
        d, max_diff, max_size = FS.pattern(name, rows, cols, T, R, rng)
        assert count(SR.filter_speckles(d, max_diff, max_size)) == components, name
    d, max_diff, max_size = FS.pattern("checkerboard", rows, cols, T, R, rng)
    r = SR.filter_speckles(d, max_diff, max_size)
    assert r["sizes"].max() == 1 and r["removed"] == (rows * cols + 1) // 2
    d, max_diff, max_size = FS.pattern("sized_pair", rows, cols, T, R, rng)
    r = SR.filter_speckles(d, max_diff, max_size)
    assert r["sizes"][R, T] == max_size and r["out"][R, T] == 0 and (r["out"][R - 2:R + 2, T - 2:T + 3] == 0).all()
    assert r["sizes"][R, 2 * T] == max_size + 1 and np.array_equal(r["out"][R - 2:R + 3, 2 * T - 2:2 * T + 3], d[R - 2:R + 3, 2 * T - 2:2 * T + 3])
    # the two blobs span four tiles each
    assert r["labels"][R + 1, T + 2] == r["labels"][R - 2, T - 2] == (R - 2) * cols + T - 2


# ---- 2. the kernels' own code, run on the host --------------------------------------------------------------------------------
def test_kernel_code_on_the_host_equals_a_flood_fill_under_sanitizers(tmp_path):
    """tests/cpp/speckle_host_main.cpp: csrc/pm_speckle_body.hpp compiled by plain g++ with -fsanitize=address,undefined.
    Maps of eight kinds at eight shapes (1x1, one pixel more than a tile either way, a tile exactly, 2 x 2 tiles and a bit)
    are labelled tile by tile in allocations of exactly a workgroup's LDS arrays; the links, merge items and flatten items
    run in forward, reverse and shuffled order; labels, sizes, output and the removed count equal a flood fill written in
    that file every time.  This covers indexing and SEQUENTIAL order-independence; it does not cover concurrent
    interleavings, which rest on the argument next to speckle_union and on the GPU tests below."""
    exe = build_host_kernel(tmp_path / "speckle_host_main", "speckle_host_main.cpp", compiler=("g++",),
                            flags=("-std=c++17", "-O1", "-Wall", "-Wextra", "-ffp-contract=off") + SANITIZE, include=(CSRC,))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "64 maps x 3 orders, 0 mismatches" in r.stdout, r.stdout + r.stderr[-3000:]
    # the program does compare: one flipped bit in an expectation is a mismatch, not a pass
    r = subprocess.run([exe, "--corrupt"], capture_output=True, text=True)
    assert r.returncode == 1 and "labels differs" in r.stderr


def test_headers_declare_and_the_library_exports_the_filter(pm):
    text = open(os.path.join(ROOT, "include", "pm", "imaging.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = pm.load()
    assert re.search(r"\bint\s+pm_filter_speckles\s*\(\s*pm_handle\s*\*", text)
    assert "typedef struct pm_speckle_filter" in text and C.sizeof(pm.PmSpeckleFilter) == 8
    for name in ("pm_filter_speckles", "pm_debug_speckle_constants"):
        assert name in pm.EXPORTS and hasattr(lib, name), name
    tile_cols, tile_rows = pm.speckle_constants()
    assert tile_cols == 64 and tile_rows >= 1  # a tile row is one wavefront


# ---- 3. device parity ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(pm):
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        yield e


def _shape(pm, name):
    T, R = pm.speckle_constants()
    return {"1x1": (1, 1), "1x(T+1)": (1, T + 1), "(R+1)x1": (R + 1, 1), "RxT": (R, T), "(R+1)x(T+1)": (R + 1, T + 1),
            "(2R+3)x(2T+5)": (2 * R + 3, 2 * T + 5), "720x1280": (720, 1280)}[name]


@functools.lru_cache(maxsize=None)
def _case(name, rows, cols, T, R):
    """(map, max_diff, max_size, the definition's result): computed once per pattern and shape, shared, never written to."""
    d, max_diff, max_size = FS.pattern(name, rows, cols, T, R, np.random.default_rng(rows * 1000 + cols))
    want = SR.filter_speckles(d, max_diff, max_size)
    for a in (d, want["out"], want["labels"], want["sizes"]):
        a.setflags(write=False)
    return d, max_diff, max_size, want


@gpu
@pytest.mark.parametrize("shape", SMALL_SHAPES)
def test_filter_equals_the_definition(pm, engine, shape):
    """Every pattern of tools/fuzz_speckle.py (constant, serpentine, comb, spiral, checkerboard, two interleaved combs, the
    max_size / max_size + 1 pair on tile corners, run maps with special values) at every small shape: out, labels, sizes
    bit for bit, the removed count through both pointers, the input untouched, guard bands intact."""
    import torch
    rows, cols = _shape(pm, shape)
    T, R = pm.speckle_constants()
    for name in FS.PATTERNS:
        d, max_diff, max_size, want = _case(name, rows, cols, T, R)
        FS.check_speckles(torch, engine, d, max_diff, max_size, want=want)


@gpu
@pytest.mark.parametrize("name", ["run_map", "constant", "serpentine"])
def test_filter_equals_the_definition_at_720x1280(pm, engine, name):
    import torch
    T, R = pm.speckle_constants()
    d, max_diff, max_size, want = _case(name, 720, 1280, T, R)
    FS.check_speckles(torch, engine, d, max_diff, max_size, want=want)


@gpu
def test_every_subset_of_the_outputs_and_of_the_removed_pointers(pm, engine):
    """Every subset of (d_out, d_labels, d_sizes), d_out == d_disp in place among them, x the removed count through the
    device pointer only, the host pointer only, both and neither (not with no other output: that is refused)."""
    import torch
    T, R = pm.speckle_constants()
    d, max_diff, max_size, want = _case("run_map", R + 1, T + 1, T, R)
    assert 0 < want["removed"] < (d > 0).sum()
    calls = 0
    for n in range(4):
        for outputs in itertools.combinations(FS.OUTPUTS, n):
            for removed in FS.REMOVED:
                if not outputs and removed == "none":
                    continue
                for inplace in ((False, True) if "out" in outputs else (False,)):
                    _, got = FS.check_speckles(torch, engine, d, max_diff, max_size, outputs, inplace, removed, want)
                    assert set(got) >= set(outputs)
                    calls += 1
    assert calls == 8 * 4 - 1 + 4 * 4


@gpu
def test_two_runs_give_identical_bytes(pm, engine):
    import torch
    T, R = pm.speckle_constants()
    for name, rows, cols in (("serpentine", 2 * R + 3, 2 * T + 5), ("run_map", 720, 1280)):
        d, max_diff, max_size, want = _case(name, rows, cols, T, R)
        first = FS.check_speckles(torch, engine, d, max_diff, max_size, want=want)[1]
        second = FS.check_speckles(torch, engine, d, max_diff, max_size, want=want)[1]
        assert first.keys() == second.keys() == {"out", "labels", "sizes", "removed", "d_removed"}
        for k in FS.OUTPUTS:
            assert np.array_equal(FC.bits(first[k]), FC.bits(second[k])), k
        assert first["removed"] == second["removed"] and first["d_removed"] == second["d_removed"]


@gpu
def test_a_planes_handle_takes_the_call(pm):
    import torch
    T, R = pm.speckle_constants()
    d, max_diff, max_size, want = _case("run_map", R + 1, T + 1, T, R)
    with pm.Engine(pm.default_params(0, patch=5, mode=pm.PM_MODE_PLANES, max_disp=24), max_rows=48, max_cols=64) as e:
        FS.check_speckles(torch, e, d, max_diff, max_size, want=want)  # PM_OK: the call reads a map, not the handle's state


@gpu
def test_the_left_map_of_a_scalar_match(pm, engine):
    """The real result of a small seeded scalar Match() (64x96): its left map filtered with max_diff 1, max_size 20 equals
    the definition on the downloaded map."""
    import torch
    import synth
    rows, cols = 64, 96
    p = synth.make_pair(7, rows=rows, cols=cols, n_points=40, dilate_factor=2)
    dl, _ = engine.match(p["left"], p["right"], p["seed_l"], p["seed_r"])
    assert dl.shape == (rows, cols) and (dl > 0).sum() > 100
    want, _ = FS.check_speckles(torch, engine, dl, 1.0, 20)
    print("Match map: %d valid pixels, %d components, %d pixels removed" % (
        (dl > 0).sum(), (want["labels"].ravel() == np.arange(rows * cols)).sum(), want["removed"]))
    FS.check_speckles(torch, engine, dl, 1.0, 20, ("out",), True, "device", want)


@gpu
def test_refused_calls_name_the_argument_and_enqueue_nothing(pm, engine):
    """Every refusal of the header: the status, the argument named in pm_last_error, d_out and the other outputs untouched."""
    import torch
    rows, cols = 16, 24
    lib, h = engine.lib, engine.h
    disp = torch.full((rows, cols), 10.0, dtype=torch.float32, device="cuda")
    outs = {k: FC.Guarded(torch, 4 * rows * cols) for k in FS.OUTPUTS}
    d_removed = FC.Guarded(torch, 4)
    host = C.c_int(-5)
    torch.cuda.synchronize()

    def call(filt=(1.0, 20), d_disp=disp.data_ptr(), r=rows, c=cols, given=True):
        f = pm.PmSpeckleFilter(*filt) if filt is not None else None
        p = lambda k: outs[k].ptr if given else None
        return lib.pm_filter_speckles(h, C.byref(f) if f is not None else None, d_disp, r, c, p("out"), p("labels"), p("sizes"),
                                      d_removed.ptr if given else None, C.byref(host) if given else None)

    def refused(rc, word, status=pm.PM_ERR_INVALID_ARG):
        text = lib.pm_last_error(h).decode()
        assert rc == status and word in text, (rc, word, text)

    refused(call(filt=None), "filter")
    refused(call(d_disp=None), "d_disp")
    refused(call(given=False), "no output")
    for max_diff in (np.nan, np.inf, -np.inf, -1.0):
        refused(call(filt=(max_diff, 20)), "max_diff")
    refused(call(filt=(1.0, -1)), "max_size")
    for r, c in ((0, cols), (rows, 0), (-1, cols), (rows, -3)):
        refused(call(r=r, c=c), "empty")
    refused(call(r=65536, c=32768), "exceed", pm.PM_ERR_SIZE)  # 2^31 pixels
    engine.synchronize()
    for buf in list(outs.values()) + [d_removed]:
        buf.read(np.uint8, 0)
    assert host.value == -5
    # the same arguments made good do run
    assert call() == pm.PM_OK and host.value == 0 and call(filt=(0.0, rows * cols)) == pm.PM_OK and host.value == rows * cols
    engine.synchronize()
    assert (outs["sizes"].read(np.int32) == rows * cols).all() and (outs["out"].read(np.float32) == 0).all()


@gpu
def test_scratch_is_owned_by_the_handle(pm):
    """The working labels and sizes are ONE handle-owned allocation through csrc/pm_devbuf.hpp: made on first use, reused at
    the same size, grown for a larger map, gone with the handle."""
    import torch
    lib = pm.load()
    live = lambda: (lib.pm_debug_live_device_allocations(), lib.pm_debug_live_device_bytes())
    before = live()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=96) as e:
        base = live()
        small = torch.full((37, 53), 3.0, dtype=torch.float32, device="cuda")
        large = torch.full((300, 500), 3.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert e.filter_speckles(small.data_ptr(), 37, 53, 1.0, 37 * 53, host_count=True) == 37 * 53
        first = live()
        assert first[0] == base[0] + 1 and first[1] - base[1] >= 8 * 37 * 53
        assert e.filter_speckles(small.data_ptr(), 37, 53, 1.0, 5, host_count=True) == 0
        assert live() == first
        assert e.filter_speckles(large.data_ptr(), 300, 500, 1.0, 300 * 500, host_count=True) == 300 * 500
        grown = live()
        assert grown[0] == first[0] and grown[1] - base[1] >= 8 * 300 * 500
        assert e.filter_speckles(small.data_ptr(), 37, 53, 1.0, 37 * 53, host_count=True) == 37 * 53
        assert live() == grown
    assert live() == before


@gpu
def test_fuzz_speckle_one_short_seeded_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_speckle.py"), "--cases", "40", "--seed", "3"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
