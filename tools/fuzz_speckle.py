"""Differential fuzz of pm_filter_speckles (through the C ABI) against its CPU definition (tests/speckle_ref.py).  Random
shapes <= 96x160 (images smaller than a tile included); maps from fuzz_normals.run_map (runs of equal values with steps,
holes and every special value of fuzz_cloud.SPECIALS), uniform random maps and the patterns below, which are the inputs
at which a tiled union-find can go wrong; max_diff from 0 to far beyond the map's range, max_size from 0 to the whole map;
every subset of the outputs, in place or not, the removed count through the device pointer, the host pointer, both or
neither.  Tolerance 0: every output bit-exact, guard bands intact, or it prints the case and exits 1.  check_speckles and
pattern are what tests/test_speckle.py runs its fixed cases through.

    python tools/fuzz_speckle.py [--cases 60] [--seed 1] [--max-rows 96] [--max-cols 160]
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import speckle_ref as SR
from fuzz_cloud import Guarded, bits, random_disp
from fuzz_normals import run_map

OUTPUTS = ("out", "labels", "sizes")
DTYPE = {"out": np.float32, "labels": np.int32, "sizes": np.int32}
REMOVED = ("none", "device", "host", "both")
PATTERNS = ("constant", "serpentine", "comb", "spiral", "checkerboard", "two_combs", "sized_pair", "run_map")


def spiral(rows, cols, value):
    """A one-pixel path that winds inwards from (0, 0) with one invalid pixel between its arms."""
    d = np.zeros((rows, cols), np.float32)
    inside = lambda y, x: 0 <= y < rows and 0 <= x < cols
    y = x = 0
    dy, dx = 0, 1
    d[0, 0] = value
    while True:
        for _ in range(2):  # straight on, or one turn to the right
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and d[ny, nx] == 0 and (not inside(ay, ax) or d[ay, ax] == 0):
                y, x = ny, nx
                d[y, x] = value
                break
            dy, dx = dx, -dy
        else:
            return d


def pattern(name, rows, cols, tile_cols, tile_rows, rng):
    """-> (disp, max_diff, max_size).  The maps of the issue that added the stage:
    constant      one component across every tile border
    serpentine    even rows valid, odd rows only at alternating ends: one component whose path crosses every border many
                  times, the deepest parent chains the merge can meet
    comb          every second column, joined only along the last row: the teeth's roots meet late
    spiral        a rectangular spiral, one component
    checkerboard  valid / invalid: all components are singletons, nothing merges
    two_combs     even columns hang from the first row at 10, odd columns stand on the last row at 20: adjacent everywhere,
                  more than max_diff apart, never joined
    sized_pair    a component of exactly max_size pixels (removed) and one of max_size + 1 (kept), each centred on a corner
                  of four tiles where the image has one, in a sea of singletons of every special value
    run_map       fuzz_normals.run_map with special values"""
    d = np.zeros((rows, cols), np.float32)
    if name == "constant":
        d[:] = 10.0
        return d, 1.0, 20
    if name == "serpentine":
        d[0::2, :] = 10.0
        d[1::4, -1] = 10.0
        d[3::4, 0] = 10.0
        return d, 1.0, 20
    if name == "comb":
        d[:, 0::2] = 10.0
        d[-1, :] = 10.0
        return d, 0.0, 20
    if name == "spiral":
        return spiral(rows, cols, 10.0), 1.0, 20
    if name == "checkerboard":
        d[(np.arange(rows)[:, None] + np.arange(cols)[None, :]) % 2 == 0] = 10.0
        return d, 1.0, 1
    if name == "two_combs":
        d[:, 0::2] = 10.0
        d[:, 1::2] = 20.0
        d[0, :] = 10.0
        d[-1, :] = 20.0
        return d, 9.5, 20
    if name == "sized_pair":
        d = random_disp(rng, rows, cols, valid=0.0, special=1.0)
        max_size = 20
        corners = [(y, x) for y in range(tile_rows, rows - 2, tile_rows) for x in range(tile_cols, cols - 2, tile_cols)]
        for k, (y, x) in enumerate(corners[:2]):  # 4 x 5 pixels around the corner, a ramp of steps of exactly max_diff
            d[y - 3:y + 3, x - 4:x + 4] = 0.0
            d[y - 2:y + 2, x - 2:x + 3] = (30.0 + 0.5 * np.arange(5, dtype=np.float32))[None, :]
            if k == 1:
                d[y + 2, x] = 31.0
        return d, 0.5, max_size
    if name == "run_map":
        return run_map(rng, rows, cols, valid=0.9, special=0.05), 1.0, 20
    raise ValueError(name)


def check_speckles(torch, e, disp, max_diff, max_size, outputs=OUTPUTS, inplace=False, removed="both", want=None):
    """One pm_filter_speckles call against the definition: the outputs named in `outputs` (inplace: d_out is d_disp), the
    removed count through the pointers `removed` names.  want: the definition's result where the caller already has it.
    Returns (definition, device results by name)."""
    rows, cols = disp.shape
    disp = np.ascontiguousarray(disp, np.float32)
    if want is None:
        want = SR.filter_speckles(disp, max_diff, max_size)
    src = Guarded(torch, 4 * rows * cols)
    src.t[src.lo:src.lo + src.n] = torch.from_numpy(disp.view(np.uint8).ravel().copy()).cuda()
    torch.cuda.synchronize()
    bufs = {k: (src if k == "out" and inplace else Guarded(torch, 4 * rows * cols)) for k in outputs}
    d_removed = Guarded(torch, 4) if removed in ("device", "both") else None
    ptr = lambda k: bufs[k].ptr if k in bufs else None
    n = e.filter_speckles(src.ptr, rows, cols, max_diff, max_size, ptr("out"), ptr("labels"), ptr("sizes"),
                          d_removed.ptr if d_removed else None, host_count=removed in ("host", "both"))
    e.synchronize()
    got = {}
    if removed in ("host", "both"):
        got["removed"] = n
    if d_removed:
        got["d_removed"] = int(d_removed.read(np.int32)[0])
    for k in ("removed", "d_removed"):
        assert k not in got or got[k] == want["removed"], "pm_filter_speckles: %s %d, definition %d" % (k, got[k], want["removed"])
    for k, buf in bufs.items():
        got[k] = buf.read(DTYPE[k]).reshape(rows, cols)
        bad = np.argwhere(bits(got[k]) != bits(want[k]))
        assert len(bad) == 0, "pm_filter_speckles: %d of %d values of %s differ; (y, x, input, got, want): %s" % (
            len(bad), got[k].size, k, [(int(y), int(x), float(disp[y, x]), float(got[k][y, x]), float(want[k][y, x])) for y, x in bad[:6]])
    if not (inplace and "out" in bufs):
        assert np.array_equal(src.read(np.uint32), bits(disp).ravel()), "pm_filter_speckles wrote to its input"
    return want, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=60)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-rows", type=int, default=96)
    ap.add_argument("--max-cols", type=int, default=160)
    a = ap.parse_args()
    import torch
    import pm_ctypes as pm
    rng = np.random.default_rng(a.seed)
    tile_cols, tile_rows = pm.speckle_constants()
    t0, components, removed = time.time(), 0, 0
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        for case in range(a.cases):
            small = rng.random() < 0.2
            rows = int(rng.integers(1, (12 if small else a.max_rows) + 1))
            cols = int(rng.integers(1, (12 if small else a.max_cols) + 1))
            kind = str(rng.choice(PATTERNS + ("run_map", "run_map", "random", "random")))
            if kind == "random":
                disp = random_disp(rng, rows, cols, valid=float(rng.choice([0.0, 0.3, 0.6, 0.95, 1.0])),
                                   special=float(rng.choice([0.0, 0.15, 0.5])))
                max_diff, max_size = 30.0, 20
            else:
                disp, max_diff, max_size = pattern(kind, rows, cols, tile_cols, tile_rows, rng)
            if rng.random() < 0.5:
                max_diff = float(rng.choice([0.0, 0.25, 1.0, 3.0, 30.0, 1e30]))
            if rng.random() < 0.5:
                max_size = int(rng.choice([0, 1, 5, 100, rows * cols]))
            how = str(rng.choice(REMOVED))
            outputs = tuple(k for k in OUTPUTS if rng.random() < 0.7)
            if not outputs and how == "none":
                outputs = ("out",)
            inplace = bool(rng.random() < 0.3)
            what = dict(case=case, rows=rows, cols=cols, kind=kind, max_diff=max_diff, max_size=max_size, outputs=outputs,
                        inplace=inplace, removed=how)
            try:
                want, _ = check_speckles(torch, e, disp, max_diff, max_size, outputs, inplace, how)
            except AssertionError as err:
                print("MISMATCH", what, err)
                sys.exit(1)
            components += int((want["labels"].ravel() == np.arange(rows * cols)).sum())
            removed += want["removed"]
    print("fuzz_speckle: %d cases (seed %d), %d components, %d pixels removed, bit-identical to the definition, %.1f s"
          % (a.cases, a.seed, components, removed, time.time() - t0))


if __name__ == "__main__":
    main()
