"""Differential fuzz of pm_filter_consistency (through the C ABI) against the CPU definition (tests/consistency_ref.py).
Random shapes <= 96x160, 1..8 sources, current maps and sources with every special value (0, -0.0, negatives, NaN, +inf,
subnormals), rigid motions from none to one that throws the whole map out of the image or behind the camera, sources that
are the current map carried along and disturbed, unrelated maps or the current map itself, options (max_diff, radius 0..2,
min_consistent, max_conflicts), every subset of the five outputs and d_out == d_disp.  Tolerance 0: the three maps and both
counts bit-exact, guard bands around every output intact, or it prints the case and exits 1.  check_consistency is what
tests/test_consistency.py runs its fixed cases through.

    python tools/fuzz_consistency.py [--cases 60] [--seed 1] [--max-rows 96] [--max-cols 160]
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import consistency_ref as CR
import reproject_ref as RR
from fuzz_cloud import Guarded, SPECIALS, bits, random_disp  # noqa: F401  (re-exported to the tests)
from fuzz_reproject import IDENTITY, random_motion, rotation  # noqa: F401

OUTPUTS = ("out", "classes", "residual", "d_counts", "counts")


def disturbed_source(cur, camera, motion, seed, noise=0.3, raise_by=4.0, set_to=2.0, zeros=0.05):
    """What source `motion` would have seen of the current map, and then got wrong: the map carried into the source's view
    (reproject_ref, close_radius 1), uniform noise of +-`noise` on its valid pixels, a box of rows/6 x cols/6 raised by
    `raise_by` (something nearer: OCCLUDED), a second box of that size set to `set_to` (seen through: CONFLICT), and `zeros`
    of the pixels without a value (UNSEEN)."""
    rows, cols = cur.shape
    rng = np.random.default_rng([int(seed), 0x5EED])  # a stream of its own: never the one that drew the current map
    s = RR.reproject(cur, camera, motion[0], motion[1], close_radius=1)["seed_l"].copy()
    s[s > 0] += rng.uniform(-noise, noise, int((s > 0).sum())).astype(np.float32)
    bh, bw = rows // 6, cols // 6
    x0 = cols // 2 - bw // 2
    y0, y1 = min(1, rows - 1), max(rows - 1 - bh, 0)  # in the bands above and below the middle, where every motion lands pixels
    s[y0:y0 + bh, x0:x0 + bw] += np.float32(raise_by)
    s[y1:y1 + bh, x0:x0 + bw] = np.float32(set_to)
    s[rng.random((rows, cols)) < zeros] = 0.0
    return s


def check_consistency(torch, e, disp, sources, camera, motions, max_diff=1.0, radius=1, min_consistent=1, max_conflicts=0,
                      outputs=OUTPUTS, in_place=False, self_source=(), want=None):
    """One pm_filter_consistency call against the definition.  outputs: which of the five are asked for; in_place: d_out is
    d_disp; self_source: indices k whose device map IS the current map's buffer (sources[k] must equal disp).  Returns the
    definition's dict."""
    rows, cols = disp.shape
    if want is None:
        want = CR.filter_consistency(disp, sources, camera, motions, max_diff, radius, min_consistent, max_conflicts)
    cur = Guarded(torch, 4 * rows * cols)
    cur.t[cur.lo:cur.lo + cur.n] = torch.from_numpy(np.ascontiguousarray(disp).view(np.uint8).ravel())
    held = [None if k in self_source else torch.from_numpy(np.ascontiguousarray(s, np.float32)).cuda() for k, s in enumerate(sources)]
    width = {"out": 4, "classes": 2, "residual": 4}
    maps = {k: Guarded(torch, width[k] * rows * cols) for k in width if k in outputs and not (k == "out" and in_place)}
    cnt = Guarded(torch, 8) if "d_counts" in outputs else None
    torch.cuda.synchronize()  # the uploads run on torch's stream, the stage on the handle's: nothing else orders them
    ptr = lambda k: maps[k].ptr if k in maps else None
    n = e.filter_consistency(camera, cur.ptr, [cur.ptr if t is None else t.data_ptr() for t in held], motions, rows, cols,
                             max_diff, radius, min_consistent, max_conflicts, cur.ptr if in_place and "out" in outputs else ptr("out"),
                             ptr("classes"), ptr("residual"), cnt.ptr if cnt else None, "counts" in outputs)
    e.synchronize()
    if "counts" in outputs:
        assert tuple(n) == tuple(int(v) for v in want["counts"]), "host counts %s, definition %s" % (n, want["counts"])
    else:
        assert n is None
    if cnt:
        got = cnt.read(np.int32)
        assert np.array_equal(got, want["counts"]), "d_counts %s, definition %s" % (got, want["counts"])
    dtypes = {"out": np.float32, "classes": np.uint16, "residual": np.float32}
    got_cur = cur.read(np.float32).reshape(rows, cols)  # its guard bands too
    if in_place and "out" in outputs:
        maps = dict(maps, out=None)
    else:
        assert np.array_equal(bits(got_cur), bits(disp)), "pm_filter_consistency wrote to its input map"
    for k, buf in maps.items():
        got = got_cur if buf is None else buf.read(dtypes[k]).reshape(rows, cols)
        w = want[k]
        same = got.view(np.uint16 if k == "classes" else np.uint32) == np.ascontiguousarray(w).view(np.uint16 if k == "classes" else np.uint32)
        bad = np.argwhere(~same)
        assert len(bad) == 0, "pm_filter_consistency: %d of %d values of %s differ; (y, x, got, want): %s" % (
            len(bad), got.size, k, [(int(y), int(x), float(got[y, x]), float(w[y, x])) for y, x in bad[:6]])
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
    t0, valid, kept = time.time(), 0, 0
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
            kw = dict(max_diff=float(rng.choice([0.0, 0.5, 1.0, hi / 4])), radius=int(rng.integers(0, 3)),
                      min_consistent=int(rng.integers(0, n + 1)), max_conflicts=int(rng.integers(0, 9)))
            outputs = tuple(k for k in OUTPUTS if rng.random() < 0.7) or ("classes",)
            in_place = bool(rng.random() < 0.3) and not self_source
            what = dict(case=case, rows=rows, cols=cols, camera=camera, n=n, sources=kinds, outputs=outputs, in_place=in_place, **kw)
            try:
                want = check_consistency(torch, e, disp, sources, camera, motions, outputs=outputs, in_place=in_place,
                                         self_source=tuple(self_source), **kw)
                valid += int(want["counts"][0])
                kept += int(want["counts"][1])
            except AssertionError as err:
                print("MISMATCH", what, err)
                sys.exit(1)
    print("fuzz_consistency: %d cases (seed %d), %d valid pixels, %d kept, bit-identical to the definition, %.1f s"
          % (a.cases, a.seed, valid, kept, time.time() - t0))


if __name__ == "__main__":
    main()
