#!/usr/bin/env python3
"""Times pm_disparity_normals (the windowed plane fit for scalar-mode maps) beside pm_backproject and the Match() whose map
it reads.

One run, one PM_MODE_SCALAR handle (bench.py's flagship parameters: 11x11 window, 8 iterations, seeded, cross-checked).  The
map is that Match()'s left map of a synthetic 1280x720 pair; at 4096x2160 the same map is tiled to the size.  Legs, each
timed with HIP events on the handle's stream around every call, median (min / max) over --steps calls after --warmup:

  match           pm_match_device, one pair per call, 1280x720
  backproject     pm_backproject of the map
  fit_r2/5/7      pm_disparity_normals, d_normals alone, max_diff 1, min_support 9 (r = 5 also at 4096x2160)
  fit_r5_all      ... with d_planes and d_support too

match and fit_r5 are timed twice, interleaved with the other legs, so that a drift of the clocks shows as a difference of the
halves.  Event times include the launch gap.  Nothing is judged: the stage is reported as a fraction of the Match, and
against the rough count of the issue (pixels x taps x ~20 lane operations).  Prints one JSON line; --record FILE writes the
table and the tree's sha (--sha) there.  With PM_LIB naming the tuning build and PM_NORMALS_FIT_RUNTIME_RADIUS=1 the fit legs
time the one-kernel variant with the radius as a launch argument (--label names the run in the record).

--only LEG [--size RxC]: that leg alone, 20 calls, no events (for a counter pass of its own under a profiler)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from bench_rectify import event_timer

CAMERA_720 = (1100.0, 1090.0, 640.3, 359.6, 0.12)  # scaled with the image for the larger size
MAX_DIFF, MIN_SUPPORT = 1.0, 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--record", default=None)
    ap.add_argument("--sha", default="unknown")
    ap.add_argument("--label", default="shipped: radius as a template constant")
    ap.add_argument("--only", default=None)
    ap.add_argument("--size", default="720x1280")
    ap.add_argument("--append", action="store_true", help="append to --record instead of replacing it")
    args = ap.parse_args()
    import torch
    import pm_ctypes as pm
    import synth
    rows, cols = 720, 1280
    res = {"steps": args.steps, "warmup": args.warmup, "label": args.label}
    with pm.Engine(pm.default_params(0, patch=11, patchmatch_iters=8), max_rows=rows, max_cols=cols) as e:
        p = synth.make_pair(0, rows, cols)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        L, R, SL, SR = up(p["left"]), up(p["right"]), up(p["seed_l"]), up(p["seed_r"])
        DL = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
        DR = torch.zeros_like(DL)
        torch.cuda.synchronize()
        match = lambda: e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), DL.data_ptr(),
                                       DR.data_ptr())
        match()
        e.synchronize()
        small = DL.cpu().numpy()
        res["match_valid_fraction"] = float((small > 0).mean())
        big_rows, big_cols = 2160, 4096
        big = np.ascontiguousarray(np.tile(small, (3, 4))[:big_rows, :big_cols])
        maps = {(rows, cols): DL.clone(), (big_rows, big_cols): up(big)}
        out = {k: (torch.empty(k + (3,), dtype=torch.float32, device="cuda"), torch.empty((3,) + k, dtype=torch.float32, device="cuda"),
                   torch.empty(k, dtype=torch.uint8, device="cuda")) for k in maps}
        torch.cuda.synchronize()

        def cam(k):
            s = k[0] / 720.0
            return tuple(v * s for v in CAMERA_720[:4]) + (CAMERA_720[4],)

        def fit(k, radius, everything=False):
            n, pl, su = out[k]
            return lambda: e.disparity_normals(cam(k), maps[k].data_ptr(), k[0], k[1], radius, MAX_DIFF, MIN_SUPPORT, n.data_ptr(),
                                               pl.data_ptr() if everything else None, su.data_ptr() if everything else None)

        s720, s2160 = (rows, cols), (big_rows, big_cols)
        legs = {
            "match": match,
            "backproject": lambda: e.backproject(cam(s720), maps[s720].data_ptr(), rows, cols, out[s720][0].data_ptr()),
            "fit_r2": fit(s720, 2), "fit_r5": fit(s720, 5), "fit_r7": fit(s720, 7), "fit_r5_all": fit(s720, 5, True),
            "fit_r5_4096x2160": fit(s2160, 5),
        }
        if args.only:
            k = tuple(int(v) for v in args.size.split("x"))
            fn = legs[args.only] if not args.only.startswith("fit_r") or k == s720 else fit(k, int(args.only[5]))
            for _ in range(20):
                fn()
            e.synchronize()
            print(json.dumps({"only": args.only, "size": args.size, "calls": 20}))
            return 0
        timed = event_timer(e, args.steps, args.warmup)
        order = ["match", "fit_r5"] + list(legs)
        res["legs"] = {}
        for name in order:
            res["legs"].setdefault(name, []).append(timed(legs[name]))
        e.synchronize()
        sup = out[s720][2].cpu().numpy()
        res["fitted_fraction"] = float((sup >= MIN_SUPPORT).mean())
    med = {k: float(np.median([r["median_ms"] for r in v])) for k, v in res["legs"].items()}
    res["median_ms"] = med
    res["fraction_of_match"] = {k: med[k] / med["match"] for k in med if k.startswith("fit_") and "x" not in k}
    print(json.dumps(res))
    if args.record:
        with open(args.record, "a" if args.append else "w") as f:
            if not args.append:
                f.write("pm_disparity_normals beside pm_backproject and the scalar Match() (tools/bench_normals_fit.py)\n")
                f.write("=" * 100 + "\n\n")
                f.write("tree: %s\n" % args.sha)
                f.write("MI355X, one PM_MODE_SCALAR handle (11x11, 8 iterations, seeded, cross-check), HIP events on the handle's\n"
                        "stream, %d calls after %d warm-up calls per leg (match and fit_r5 timed twice, interleaved).  The map: the\n"
                        "left map of that Match() of a synthetic 1280x720 pair, %.1f %% of its pixels > 0 (%.1f %% get a fit at\n"
                        "r = 5); tiled to 4096x2160.  max_diff %.1f, min_support %d; fit legs write d_normals alone, fit_r5_all\n"
                        "all three outputs.\n" % (args.steps, args.warmup, 100 * res["match_valid_fraction"],
                                                  100 * res["fitted_fraction"], MAX_DIFF, MIN_SUPPORT))
            f.write("\n[%s]  ms:\n" % args.label)
            for k, rs in res["legs"].items():
                for r in rs:
                    f.write("  %-18s median %.4f  min %.4f  max %.4f\n" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
            f.write("  as a fraction of the one-pair Match (%.3f ms): %s\n"
                    % (med["match"], ", ".join("%s %.3f" % (k, v) for k, v in res["fraction_of_match"].items())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
