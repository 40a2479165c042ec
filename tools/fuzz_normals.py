"""Differential fuzz of pm_disparity_normals (through the C ABI) against its CPU definition (tests/normals_fit_ref.py).
Random shapes <= 96x160 (images smaller than the window included), radii 1..7, maps from empty to full with every special
value of fuzz_cloud.SPECIALS, runs of equal values and steps (what a scalar-mode match leaves), max_diff from 0 to far
beyond the map's range, min_support from 3 to the whole window, cameras, destination alignments and every non-empty subset
of the three outputs.  Tolerance 0: bit-exact, guard bands around every output intact, or it prints the case and exits 1.
check_normals_fit is what tests/test_normals_fit.py runs its fixed cases through.

    python tools/fuzz_normals.py [--cases 60] [--seed 1] [--max-rows 96] [--max-cols 160]
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import normals_fit_ref as NR
from fuzz_cloud import Guarded, bits, random_disp

OUTPUTS = ("normals", "planes", "support")
WIDTH = {"normals": 12, "planes": 12, "support": 1}  # bytes per pixel


def run_map(rng, rows, cols, valid=0.9, special=0.02):
    """A slanted plane quantised into runs of 1..8 equal values along rows, with holes and special values: the shape of a
    scalar-mode result."""
    a, b, c = rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), rng.uniform(20.0, 60.0)
    x = np.arange(cols)[None, :]
    y = np.arange(rows)[:, None]
    d = (c + a * (x - cols / 2) + b * (y - rows / 2)).astype(np.float32)
    for r in range(rows):
        k = 0
        while k < cols:
            n = int(rng.integers(1, 9))
            d[r, k:k + n] = d[r, k]
            k += n
    d[rng.random((rows, cols)) >= valid] = 0.0
    pick = rng.random((rows, cols)) < special
    d[pick] = random_disp(rng, rows, cols, valid=0.0, special=1.0)[pick]
    return d


def check_normals_fit(torch, e, disp, camera, radius, max_diff, min_support, outputs=OUTPUTS, offset_floats=0, want=None):
    """One pm_disparity_normals call against the definition: the outputs named in `outputs`, d_normals `offset_floats`
    floats past a 16-byte boundary.  want: the definition's result for these arguments where the caller already has it.
    Returns the device results by name."""
    rows, cols = disp.shape
    if want is None:
        want = NR.disparity_normals(disp, camera, radius, max_diff, min_support)
    d = torch.from_numpy(np.ascontiguousarray(disp, np.float32)).cuda()
    bufs = {k: Guarded(torch, WIDTH[k] * rows * cols, 4 * offset_floats if k == "normals" else 0) for k in outputs}
    ptr = lambda k: bufs[k].ptr if k in bufs else None
    e.disparity_normals(camera if "normals" in bufs else None, d.data_ptr(), rows, cols, radius, max_diff, min_support,
                        ptr("normals"), ptr("planes"), ptr("support"))
    e.synchronize()
    got = {}
    for k, buf in bufs.items():
        g = buf.read(np.uint8 if k == "support" else np.float32)
        got[k] = g.reshape(want[k].shape)
        bad = np.argwhere(bits(got[k]) != bits(want[k]))
        assert len(bad) == 0, "pm_disparity_normals: %d of %d values of %s differ; (index, got, want): %s" % (
            len(bad), g.size, k, [(tuple(int(v) for v in i), float(got[k][tuple(i)]), float(want[k][tuple(i)])) for i in bad[:6]])
    return got


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
    t0, fits = time.time(), 0
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        for case in range(a.cases):
            small = rng.random() < 0.2
            rows = int(rng.integers(1, (12 if small else a.max_rows) + 1))
            cols = int(rng.integers(1, (12 if small else a.max_cols) + 1))
            f = float(rng.uniform(0.4, 2.0) * cols)
            camera = (f * float(rng.choice([1.0, -1.0], p=[0.9, 0.1])), f * float(rng.uniform(0.8, 1.25)),
                      cols / 2 + float(rng.normal(0, 3)), rows / 2 + float(rng.normal(0, 3)), float(rng.uniform(0.02, 0.5)))
            if rng.random() < 0.5:
                disp = run_map(rng, rows, cols, valid=float(rng.choice([0.3, 0.9, 1.0])), special=float(rng.choice([0.0, 0.05])))
            else:
                disp = random_disp(rng, rows, cols, valid=float(rng.choice([0.0, 0.05, 0.3, 0.95, 1.0])),
                                   special=float(rng.choice([0.0, 0.15, 0.5])))
            radius = int(rng.integers(1, 8))
            window = (2 * radius + 1) ** 2
            kw = dict(radius=radius, max_diff=float(rng.choice([0.0, 0.25, 1.0, 3.0, 30.0, 1e30])),
                      min_support=int(rng.choice([3, 3, 9, window // 2, window])))
            outputs = ()
            while not outputs:
                outputs = tuple(k for k in OUTPUTS if rng.random() < 0.7)
            offset = int(rng.integers(0, 4))
            what = dict(case=case, rows=rows, cols=cols, camera=camera, outputs=outputs, offset=offset, **kw)
            try:
                got = check_normals_fit(torch, e, disp, camera, outputs=outputs, offset_floats=offset, **kw)
            except AssertionError as err:
                print("MISMATCH", what, err)
                sys.exit(1)
            if "support" in got:
                fits += int((got["support"] >= kw["min_support"]).sum())
    print("fuzz_normals: %d cases (seed %d), %d pixels with enough support, bit-identical to the definition, %.1f s"
          % (a.cases, a.seed, fits, time.time() - t0))


if __name__ == "__main__":
    main()
