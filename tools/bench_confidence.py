#!/usr/bin/env python3
"""Times pm_disparity_confidence beside its yardstick: the engine's own cost kernels, measured in the same run on the Match()
that made the map.

The map is a REAL match's: a scalar pm_match_device (8 iterations, the default 11x11 window, cross-check on) of the benchmark's
synthetic pair at 1280x720 and at 4096x2160, standard seeds, with pm_profile on.  From that profile, per launch:

  t_noise       PM_K_NOISE        one lerped window evaluation per positive pixel (k_noise_cost_tiled)
  t_background  PM_K_BACKGROUND   one byte SAD plus, uncached, one lerped evaluation (k_background_tiled)

The stage does three lerped evaluations, one byte SAD and two Sobel gradients per measured pixel, so the figure reported is

  t_conf / (3 t_noise + t_background)

per leg.  Near or under 1 says that staging the tile once for all four evaluations pays; well above 1 says what to look at
next.  REPORTED, not a gate: the exit status is 0 either way.

Legs, each timed with HIP events on the handle's stream around every call (the 16-byte memset, the gradient launch, the main
launch and the 12-byte copy of the counts), median (min / max) over --steps calls after --warmup, every leg TWICE, interleaved,
so that a drift of the clocks shows as a difference of the halves:

  all           every output (d_out, d_measures, d_flags, d_counts), with the right map
  all_no_right  the same without d_disp_r
  flags         d_flags and d_counts alone, with the right map

Every leg passes device counts and no host counts: nothing synchronises inside the timed window.  Thresholds: max_cost 10,
min_margin 2, min_bg_margin 5, max_lr_diff 1; window 11x11.

Prints one JSON line; --record FILE writes the times and the ratios there, stamped with --sha."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from bench_cloud import SIZES
from bench_rectify import event_timer

PATCH = 11
THRESHOLDS = dict(max_cost=10.0, min_margin=2.0, min_bg_margin=5.0, max_lr_diff=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--record", default=None)
    ap.add_argument("--sha", default="unknown")
    ap.add_argument("--sizes", default=None, help="e.g. 720x1280 (rows x cols); default: both")
    args = ap.parse_args()
    import torch
    import pm_ctypes as pm
    import synth
    sizes = SIZES if not args.sizes else tuple(tuple(int(v) for v in s.split("x")) for s in args.sizes.split(","))
    res = {"steps": args.steps, "warmup": args.warmup, "patch": PATCH, "sizes": {}}
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for rows, cols in sizes:
        pair = synth.make_pair(0, rows, cols)
        L, R, SL, SR = up(pair["left"]), up(pair["right"]), up(pair["seed_l"]), up(pair["seed_r"])
        D = torch.zeros((2, rows, cols), dtype=torch.float32, device="cuda")
        out = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
        meas = torch.empty((4, rows, cols), dtype=torch.float32, device="cuda")
        flags = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros((3,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pm.Engine(pm.default_params(0, patch=PATCH, patchmatch_iters=8), max_rows=rows, max_cols=cols) as e:
            match = lambda: e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), D[0].data_ptr(),
                                           D[1].data_ptr())
            match()  # warm: allocations, code objects
            e.synchronize()
            e.profile_enable(True)
            match()
            e.synchronize()
            prof = e.profile_read()
            e.profile_enable(False)
            per_launch = {k: (prof[k][1] / prof[k][0] if prof[k][0] else float("nan")) for k in ("noise_cost", "background")}
            yard = 3 * per_launch["noise_cost"] + per_launch["background"]

            def conf(outputs, right=True, host=False):
                full = outputs == "all"
                return e.disparity_confidence(L.data_ptr(), R.data_ptr(), D[0].data_ptr(), D[1].data_ptr() if right else None, rows,
                                              cols, PATCH, d_out=out.data_ptr() if full else None,
                                              d_measures=meas.data_ptr() if full else None, d_flags=flags.data_ptr(),
                                              d_counts=d_cnt.data_ptr(), want_counts=host, **THRESHOLDS)

            counts = conf("all", host=True)  # and the scratch, outside the timing
            legs = {"all": lambda: conf("all"), "all_no_right": lambda: conf("all", right=False), "flags": lambda: conf("flags")}
            timed = event_timer(e, args.steps, args.warmup)
            o = {"pixels": rows * cols, "counts": counts, "profile_launches": {k: prof[k][0] for k in per_launch},
                 "per_launch_ms": per_launch, "yardstick_ms": yard, "legs": {}}
            for name in list(legs) + list(legs):  # every leg twice, interleaved
                o["legs"].setdefault(name, []).append(timed(legs[name]))
            e.synchronize()
            o["median_ms"] = {k: float(np.median([r["median_ms"] for r in v])) for k, v in o["legs"].items()}
            o["ratio"] = {k: v / yard for k, v in o["median_ms"].items()}
            res["sizes"]["%dx%d" % (cols, rows)] = o
    print(json.dumps(res))
    if args.record:
        with open(args.record, "w") as f:
            f.write("pm_disparity_confidence beside the engine's own cost kernels (tools/bench_confidence.py)\n" + "=" * 100 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            f.write("MI355X, one handle, HIP events on the handle's stream, same run, %d calls after %d warm-up calls per leg, every leg\n"
                    "timed twice, interleaved.  The maps: a real scalar match (8 iterations, %dx%d window, cross-check) of the benchmark's\n"
                    "synthetic pair at each size; pm_profile of THAT match gives the yardstick, per launch.  Thresholds 10 / 2 / 5 / 1.\n"
                    "Reported, not a gate.\n\n" % (args.steps, args.warmup, PATCH, PATCH))
            for size, o in res["sizes"].items():
                c = o["counts"]
                f.write("%s: %d pixels; valid %d, measured %d, kept %d; ms:\n" % (size, o["pixels"], c[0], c[1], c[2]))
                f.write("  PM_K_NOISE       %.4f per launch (%d launches)\n" % (o["per_launch_ms"]["noise_cost"], o["profile_launches"]["noise_cost"]))
                f.write("  PM_K_BACKGROUND  %.4f per launch (%d launches)\n" % (o["per_launch_ms"]["background"], o["profile_launches"]["background"]))
                f.write("  yardstick 3 t_noise + t_background = %.4f\n" % o["yardstick_ms"])
                for k, rs in o["legs"].items():
                    for r in rs:
                        f.write("  %-13s median %.4f  min %.4f  max %.4f\n" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
                for k, v in o["ratio"].items():
                    f.write("  t_%s %.4f / yardstick %.4f = %.3f\n" % (k, o["median_ms"][k], o["yardstick_ms"], v))
                f.write("\n")
            f.write("Event times include the launch gaps (a memset, two launches and a copy against one launch of the yardstick's kernels).\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
