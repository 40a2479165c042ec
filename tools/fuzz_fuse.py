"""Differential fuzz of pm_fuse_disparity (through the C ABI) against the CPU definition (tests/fuse_ref.py).  Random shapes
<= 96x160, 1..8 sources, current maps and sources with every special value (0, -0.0, negatives, NaN, +inf, subnormals), rigid
motions from none to one that throws the whole map out of the image or behind the camera, sources that are the current map
carried along and disturbed, unrelated maps or the current map itself, weight planes that are absent, partly absent or hold 0,
negatives, NaN and +-inf, options (max_diff, radius 0..2, min_consistent, max_conflicts, fill_min_sources, fill_max_diff),
every subset of the six outputs and d_out == d_disp.  Tolerance 0: the four maps and the four counts bit-exact, guard bands
around every output intact, or it prints the case and exits 1.  check_fuse is what tests/test_fuse.py runs its fixed cases
through.

    python tools/fuzz_fuse.py [--cases 60] [--seed 1] [--max-rows 96] [--max-cols 160]
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import fuse_ref as FU
from fuzz_cloud import Guarded, SPECIALS, bits, random_disp  # noqa: F401  (re-exported to the tests)
from fuzz_consistency import disturbed_source  # noqa: F401
from fuzz_reproject import IDENTITY, random_motion, rotation  # noqa: F401

OUTPUTS = ("out", "count", "spread", "flags", "d_counts", "counts")
WIDTH = {"out": 4, "count": 1, "spread": 4, "flags": 1}
DTYPE = {"out": np.float32, "count": np.uint8, "spread": np.float32, "flags": np.uint8}
WEIGHT_SPECIALS = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-45, 0.25, 3.0], np.float32)


def random_weight(rng, rows, cols, special=0.2):
    """A weight plane in (0.1, 4) with `special` of its pixels drawn from WEIGHT_SPECIALS."""
    w = rng.uniform(0.1, 4.0, (rows, cols)).astype(np.float32)
    pick = rng.random((rows, cols)) < special
    w[pick] = rng.choice(WEIGHT_SPECIALS, int(pick.sum()))
    return w


def check_fuse(torch, e, disp, sources, camera, motions, weight=None, source_weights=None, max_diff=1.0, radius=1,
               min_consistent=1, max_conflicts=0, fill_min_sources=0, fill_max_diff=1.0, outputs=OUTPUTS, in_place=False,
               self_source=(), offset_floats=0, array_of_nulls=False, want=None):
    """One pm_fuse_disparity call against the definition.  outputs: which of the six are asked for; in_place: d_out is
    d_disp; self_source: indices k whose device map IS the current map's buffer (sources[k] must equal disp); offset_floats:
    the current map, the sources, the weights and the float outputs start that many floats past a 16-byte boundary;
    array_of_nulls: where no source has weights, d_source_weights is an array of nulls instead of null.  Returns the
    definition's dict."""
    rows, cols = disp.shape
    n = len(sources)
    if source_weights is None:
        source_weights = [None] * n
    if want is None:
        want = FU.fuse(disp, sources, camera, motions, weight, source_weights, max_diff, radius, min_consistent, max_conflicts,
                       fill_min_sources, fill_max_diff)
    off = 4 * offset_floats

    def up(a):
        t = torch.zeros(rows * cols + offset_floats, dtype=torch.float32, device="cuda")
        t[offset_floats:] = torch.from_numpy(np.ascontiguousarray(a, np.float32).ravel())
        return t

    cur = Guarded(torch, 4 * rows * cols, off)
    cur.t[cur.lo:cur.lo + cur.n] = torch.from_numpy(np.ascontiguousarray(disp).view(np.uint8).ravel())
    held = [None if k in self_source else up(s) for k, s in enumerate(sources)]
    w_cur = up(weight) if weight is not None else None
    w_src = [up(w) if w is not None else None for w in source_weights]
    maps = {k: Guarded(torch, WIDTH[k] * rows * cols, off if WIDTH[k] == 4 else offset_floats)
            for k in WIDTH if k in outputs and not (k == "out" and in_place)}
    cnt = Guarded(torch, 16) if "d_counts" in outputs else None
    torch.cuda.synchronize()  # the uploads run on torch's stream, the stage on the handle's: nothing else orders them
    ptr = lambda k: maps[k].ptr if k in maps else None
    got_n = e.fuse_disparity(camera, cur.ptr, [cur.ptr if t is None else t.data_ptr() + off for t in held], motions, rows, cols,
                             max_diff, radius, min_consistent, max_conflicts, fill_min_sources, fill_max_diff,
                             w_cur.data_ptr() + off if w_cur is not None else None,
                             None if all(w is None for w in w_src) and not array_of_nulls else [w.data_ptr() + off if w is not None else None for w in w_src],
                             cur.ptr if in_place and "out" in outputs else ptr("out"), ptr("count"), ptr("spread"), ptr("flags"),
                             cnt.ptr if cnt else None, "counts" in outputs)
    e.synchronize()
    if "counts" in outputs:
        assert tuple(got_n) == tuple(int(v) for v in want["counts"]), "host counts %s, definition %s" % (got_n, want["counts"])
    else:
        assert got_n is None
    if cnt:
        got = cnt.read(np.int32)
        assert np.array_equal(got, want["counts"]), "d_counts %s, definition %s" % (got, want["counts"])
    got_cur = cur.read(np.float32).reshape(rows, cols)  # its guard bands too
    if in_place and "out" in outputs:
        maps = dict(maps, out=None)
    else:
        assert np.array_equal(bits(got_cur), bits(disp)), "pm_fuse_disparity wrote to its input map"
    for k, buf in maps.items():
        got = got_cur if buf is None else buf.read(DTYPE[k]).reshape(rows, cols)
        w = np.ascontiguousarray(want[k])
        bad = np.argwhere(bits(got) != bits(w))
        assert len(bad) == 0, "pm_fuse_disparity: %d of %d values of %s differ; (y, x, input, got, want): %s" % (
            len(bad), got.size, k, [(int(y), int(x), float(disp[y, x]), float(got[y, x]), float(w[y, x])) for y, x in bad[:6]])
    return want


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
    t0, totals = time.time(), np.zeros(4, np.int64)
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        for case in range(a.cases):
            rows, cols = int(rng.integers(1, a.max_rows + 1)), int(rng.integers(1, a.max_cols + 1))
            f = float(rng.uniform(0.4, 2.0) * cols)
            camera = (f, f * float(rng.uniform(0.8, 1.25)), cols / 2 + float(rng.normal(0, 3)), rows / 2 + float(rng.normal(0, 3)),
                      float(rng.uniform(0.02, 0.5)))
            hi = float(rng.choice([4.0, 30.0, 90.0]))
            disp = random_disp(rng, rows, cols, valid=float(rng.choice([0.05, 0.5, 0.95, 1.0])),
                               special=float(rng.choice([0.0, 0.1, 0.5])), hi=hi)
            if rng.random() < 0.5:  # piecewise constant: surfaces instead of noise
                disp[disp > 0] = np.round(disp[disp > 0] / (hi / 3)) * np.float32(hi / 3) + np.float32(0.5)
            n = int(rng.integers(1, pm.PM_CONSISTENCY_MAX_SOURCES + 1))
            kinds, motions, sources, self_source = [], [], [], []
            for k in range(n):
                kind, motion = random_motion(rng, camera, camera[0] * camera[4] / (hi / 2))
                how = rng.choice(["carried", "carried", "unrelated", "self"])
                if how == "carried":
                    clean = np.where(np.isfinite(disp) & (disp > 0), disp, 0).astype(np.float32)
                    clean[clean == 0] = np.float32(hi / 3)  # the source still sees what the current map lost: something to fill
                    s = disturbed_source(clean, camera, motion, int(rng.integers(1 << 30)), noise=float(rng.choice([0.0, 0.3])))
                    pick = rng.random((rows, cols)) < 0.03
                    s[pick] = rng.choice(SPECIALS, int(pick.sum()))
                elif how == "unrelated":
                    s = random_disp(rng, rows, cols, valid=0.8, special=0.1, hi=hi)
                else:
                    s = disp
                    self_source.append(k)
                kinds.append("%s/%s" % (kind, how))
                motions.append(motion)
                sources.append(s)
            weight = random_weight(rng, rows, cols) if rng.random() < 0.5 else None
            source_weights = [random_weight(rng, rows, cols) if rng.random() < 0.5 else None for _ in range(n)]
            kw = dict(max_diff=float(rng.choice([0.0, 0.5, 1.0, hi / 4])), radius=int(rng.integers(0, 3)),
                      min_consistent=int(rng.integers(0, n + 1)), max_conflicts=int(rng.integers(0, 9)),
                      fill_min_sources=int(rng.integers(0, n + 1)), fill_max_diff=float(rng.choice([0.0, 0.5, hi / 4])))
            outputs = tuple(k for k in OUTPUTS if rng.random() < 0.7) or ("flags",)
            in_place = bool(rng.random() < 0.3) and not self_source
            what = dict(case=case, rows=rows, cols=cols, camera=camera, n=n, sources=kinds, outputs=outputs, in_place=in_place,
                        weight=weight is not None, source_weights=[w is not None for w in source_weights], **kw)
            try:
                want = check_fuse(torch, e, disp, sources, camera, motions, weight, source_weights, outputs=outputs,
                                  in_place=in_place, self_source=tuple(self_source), offset_floats=int(rng.integers(0, 4)),
                                  array_of_nulls=bool(rng.random() < 0.5), **kw)
                totals += want["counts"]
            except AssertionError as err:
                print("MISMATCH", what, err)
                sys.exit(1)
    print("fuzz_fuse: %d cases (seed %d), %d valid pixels, %d kept, %d fused, %d filled, bit-identical to the definition, %.1f s"
          % (a.cases, a.seed, *totals, time.time() - t0))


if __name__ == "__main__":
    main()
