"""Differential fuzz of pm_disparity_confidence (through the C ABI) against the CPU definition (tests/confidence_ref.py).
Random shapes <= 40x160, windows 3..15 a side (square or not), synthetic pairs, left maps from near the ground truth to
uniform noise with every special value (0, -0.0, negatives, NaN, +inf, subnormals) and values beyond the measured domain,
right maps or none, thresholds from -inf to +inf, drop_unmeasured both ways, every subset of the five outputs and
d_out == d_disp_l.  Tolerance 0: the map, the four measures, the flags and the three counts bit-exact, guard bands around
every output intact, or it prints the case and exits 1.  check_confidence is what tests/test_confidence.py runs its fixed
cases through; disturbed_case builds them.

    python tools/fuzz_confidence.py [--cases 40] [--seed 1] [--max-rows 40] [--max-cols 160]
"""
import argparse, functools, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import confidence_ref as CF
import oracle_lib as O
import synth
from fuzz_cloud import Guarded, SPECIALS, bits  # noqa: F401  (re-exported to the tests)

OUTPUTS = ("out", "measures", "flags", "d_counts", "counts")
THRESHOLDS = dict(max_cost=10.0, min_margin=2.0, min_bg_margin=5.0, max_lr_diff=1.0)  # at which every verdict occurs


@functools.lru_cache(maxsize=None)
def matched_pair(rows, cols, pw, ph):
    """synth.make_pair(0, rows, cols, d_max, n_points) and its oracle Match(): 3 iterations of the pw x ph window, with the
    cross-check -> (left, right, disp_l, disp_r).  A shape the window does not fit keeps the seeds."""
    d_max = max(4.0, min(24.0, cols / 4.0))
    p = synth.make_pair(0, rows=rows, cols=cols, d_max=d_max, n_points=max(4, rows * cols // 60), dilate_factor=2)
    prm = O.default_params(O.SEM_CPU, n_iters=3, nthreads=4, left_right_check=1)
    for i in range(3):
        prm.patch_w[i], prm.patch_h[i] = pw, ph
    prm.bg_patch_w, prm.bg_patch_h = pw, ph
    if rows >= ph and cols >= pw:
        dl, dr = O.match(prm, p["left"], p["right"], p["seed_l"], p["seed_r"])
    else:
        dl, dr = p["seed_l"].copy(), p["seed_r"].copy()
    return p["left"], p["right"], dl, dr


def disturbed_case(rows, cols, pw, ph):
    """matched_pair with the left map disturbed so that every verdict occurs: the positive pixels of the right third of the
    columns shifted by +2.5, four middle rows shifted by -0.75 and floored at 0.25."""
    left, right, dl, dr = matched_pair(rows, cols, pw, ph)
    dl = dl.copy()
    third = np.zeros(dl.shape, bool)
    third[:, (2 * cols) // 3:] = True
    dl[third & (dl > 0)] += np.float32(2.5)
    y0 = max(rows // 2 - 2, 0)
    band = np.zeros(dl.shape, bool)
    band[y0:y0 + 4] = True
    pick = band & (dl > 0)
    dl[pick] = np.maximum(dl[pick] - np.float32(0.75), np.float32(0.25))
    return left, right, dl, dr


def ramp_case(rows, cols, pw):
    """A map whose tiles span more target columns than the LDS holds: d = 1 in even columns and x - pw / 2 - 1 in odd ones."""
    left, right, _, dr = matched_pair(rows, cols, pw, pw)
    x = np.arange(cols, dtype=np.float32)[None, :].repeat(rows, 0)
    dl = np.where(np.arange(cols)[None, :] % 2 == 0, np.float32(1.0), np.maximum(x - np.float32(pw // 2 + 1), np.float32(0.5)))
    return left, right, np.ascontiguousarray(dl, np.float32), dr


def fallback_tiles(disp_l, measured, pw, constants):
    """The tiles of a case that take the global-memory path, by the rule include/pm/testing.h states."""
    tw, th, target = constants
    rows, cols = measured.shape
    n = 0
    for y0 in range(0, rows, th):
        for x0 in range(0, cols, tw):
            ys, xs = np.nonzero(measured[y0:y0 + th, x0:x0 + tw])
            if len(ys) == 0:
                continue
            xs, ys = xs + x0, ys + y0
            d = disp_l[ys, xs]
            xf = xs.astype(np.float32)
            dp = d + np.float32(1.0)
            dd = np.where(dp <= xf - np.float32(pw // 2), dp, d).astype(np.float32)
            cx = (xf - dd) - np.float32((pw - 1) * 0.5)
            lo4 = int(np.floor(cx).min()) & ~3
            n += int(lo4 + target < int(xs.max()) - pw // 2 + pw + 1)
    return n


def check_confidence(torch, e, left, right, disp_l, disp_r, pw=5, ph=None, outputs=OUTPUTS, in_place=False, want=None,
                     image_offset=0, **opts):
    """One pm_disparity_confidence call against the definition.  outputs: which of the five are asked for; in_place: d_out is
    d_disp_l; image_offset: bytes by which the two image pointers are moved off their allocation's alignment.  opts: the
    thresholds and drop_unmeasured.  Returns the definition's dict."""
    ph = pw if ph is None else ph
    disp_l = np.ascontiguousarray(disp_l, np.float32)
    rows, cols = disp_l.shape
    if want is None:
        want = CF.confidence(left, right, disp_l, disp_r, pw, ph, functor=(e.params.functor_alpha, e.params.functor_tau_color,
                                                                          e.params.functor_tau_grad), **opts)
    up = lambda a, off=0: (Guarded(torch, a.nbytes, off), np.ascontiguousarray(a).view(np.uint8).ravel())
    bufs = {}
    for k, a, off in (("left", left, image_offset), ("right", right, image_offset), ("dl", disp_l, 0)) + (
            (("dr", disp_r, 0),) if disp_r is not None else ()):
        g, raw = up(a, off)
        g.t[g.lo:g.lo + g.n] = torch.from_numpy(raw.copy())
        bufs[k] = g
    width = {"out": 4, "measures": 16, "flags": 1}
    maps = {k: Guarded(torch, width[k] * rows * cols) for k in width if k in outputs and not (k == "out" and in_place)}
    cnt = Guarded(torch, 12) if "d_counts" in outputs else None
    torch.cuda.synchronize()  # the uploads run on torch's stream, the stage on the handle's: nothing else orders them
    ptr = lambda k: maps[k].ptr if k in maps else None
    n = e.disparity_confidence(bufs["left"].ptr, bufs["right"].ptr, bufs["dl"].ptr, bufs["dr"].ptr if "dr" in bufs else None,
                               rows, cols, pw, ph, d_out=bufs["dl"].ptr if in_place and "out" in outputs else ptr("out"),
                               d_measures=ptr("measures"), d_flags=ptr("flags"), d_counts=cnt.ptr if cnt else None,
                               want_counts="counts" in outputs, **opts)
    e.synchronize()
    if "counts" in outputs:
        assert tuple(n) == tuple(int(v) for v in want["counts"]), "host counts %s, definition %s" % (n, want["counts"])
    else:
        assert n is None
    if cnt:
        got = cnt.read(np.int32)
        assert np.array_equal(got, want["counts"]), "d_counts %s, definition %s" % (got, want["counts"])
    for k, a in (("left", left), ("right", right)) + ((("dr", disp_r),) if disp_r is not None else ()):
        assert np.array_equal(bufs[k].read(np.uint8), np.ascontiguousarray(a).view(np.uint8).ravel()), "%s was written" % k
    got_dl = bufs["dl"].read(np.float32).reshape(rows, cols)  # its guard bands too
    if in_place and "out" in outputs:
        maps = dict(maps, out=None)
    else:
        assert np.array_equal(bits(got_dl), bits(disp_l)), "pm_disparity_confidence wrote to its input map"
    dtypes = {"out": np.float32, "measures": np.float32, "flags": np.uint8}
    for k, buf in maps.items():
        w = want[k]
        got = got_dl if buf is None else buf.read(dtypes[k]).reshape(w.shape)
        bad = np.argwhere(bits(got) != bits(w))
        assert len(bad) == 0, "pm_disparity_confidence: %d of %d values of %s differ; (index, d, got, want): %s" % (
            len(bad), got.size, k, [(tuple(int(v) for v in i), float(disp_l[tuple(i[-2:])]), float(got[tuple(i)]), float(w[tuple(i)]))
                                    for i in bad[:6]])
    return want


def random_map(rng, left, right, dl, cols, pw):
    """A left map for a fuzz case: the matched one, disturbed by noise, mixed with uniform values, special values and values
    next to the ends of the measured domain."""
    rows = dl.shape[0]
    d = dl.copy()
    how = rng.choice(["matched", "noisy", "uniform"])
    if how == "noisy":
        d[d > 0] += rng.uniform(-1.5, 1.5, int((d > 0).sum())).astype(np.float32)
    elif how == "uniform":
        d = rng.uniform(0.0, max(cols / 2.0, 2.0), d.shape).astype(np.float32)
    x = np.arange(cols, dtype=np.float32)[None, :].repeat(rows, 0)
    hi = x - np.float32(pw // 2)
    for value in (hi, hi - np.float32(0.5), hi + np.float32(0.5), hi - np.float32(1.0), np.float32(1.0), np.float32(0.5)):
        pick = rng.random(d.shape) < 0.02
        d[pick] = np.broadcast_to(value, d.shape)[pick]
    pick = rng.random(d.shape) < float(rng.choice([0.0, 0.05, 0.3]))
    d[pick] = rng.choice(SPECIALS, int(pick.sum()))
    return d, how


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-rows", type=int, default=40)
    ap.add_argument("--max-cols", type=int, default=160)
    a = ap.parse_args()
    import torch
    import pm_ctypes as pm
    rng = np.random.default_rng(a.seed)
    t0, measured, kept = time.time(), 0, 0
    inf = float("inf")
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        for case in range(a.cases):
            rows, cols = int(rng.integers(1, a.max_rows + 1)), int(rng.integers(1, a.max_cols + 1))
            pw = int(rng.choice([3, 5, 7, 9, 11, 13, 15]))
            ph = pw if rng.random() < 0.6 else int(rng.choice([3, 5, 7, 9, 11, 13, 15]))
            p = synth.make_pair(int(rng.integers(1 << 20)), rows=rows, cols=cols, d_max=max(4.0, cols / 4.0), n_points=8)
            dl, how = random_map(rng, p["left"], p["right"], np.where(rng.random((rows, cols)) < 0.8, p["gt"], 0).astype(np.float32),
                                 cols, pw)
            dr = None
            if rng.random() < 0.6:
                dr = p["gt"][:, ::-1].copy() if rng.random() < 0.3 else rng.uniform(0.0, cols / 3.0 + 1, (rows, cols)).astype(np.float32)
                pick = rng.random(dr.shape) < 0.1
                dr[pick] = rng.choice(SPECIALS, int(pick.sum()))
            opts = dict(max_cost=float(rng.choice([inf, 10.0, 3.0, -inf])), min_margin=float(rng.choice([-inf, 2.0, 0.0, inf])),
                        min_bg_margin=float(rng.choice([-inf, 5.0, 0.0, inf])), max_lr_diff=float(rng.choice([inf, 1.0, 0.0, -inf])),
                        drop_unmeasured=int(rng.integers(0, 2)))
            outputs = tuple(k for k in OUTPUTS if rng.random() < 0.7) or ("flags",)
            in_place = bool(rng.random() < 0.3)
            what = dict(case=case, rows=rows, cols=cols, pw=pw, ph=ph, map=how, right=dr is not None, outputs=outputs,
                        in_place=in_place, **opts)
            try:
                want = check_confidence(torch, e, p["left"], p["right"], dl, dr, pw, ph, outputs=outputs, in_place=in_place,
                                        image_offset=int(rng.integers(0, 4)), **opts)
                measured += int(want["counts"][1])
                kept += int(want["counts"][2])
            except AssertionError as err:
                print("MISMATCH", what, err)
                sys.exit(1)
    print("fuzz_confidence: %d cases (seed %d), %d measured pixels, %d kept, bit-identical to the definition, %.1f s"
          % (a.cases, a.seed, measured, kept, time.time() - t0))


if __name__ == "__main__":
    main()
