#!/usr/bin/env python3
"""Times pm_filter_speckles (the connected-component speckle filter) beside the Match() whose map it reads and beside
pm_disparity_normals at r = 7, the costliest post-Match stage before it.

One run, one PM_MODE_SCALAR handle (bench.py's flagship parameters: 11x11 window, 8 iterations, seeded, cross-checked), all
at 1280x720.  Legs, each timed with HIP events on the handle's stream around every call, median (min / max) over --steps
calls after --warmup:

  match              pm_match_device, one pair per call
  speckle_match      pm_filter_speckles of that Match()'s left map: d_out, d_labels, d_sizes and d_removed, not in place
  speckle_match_out  ... d_out alone, in place is not timed (the map would change from call to call)
  speckle_serpentine the same call on the serpentine of tools/fuzz_speckle.py: one component whose path crosses every tile
                     border, the worst case for parent chains
  speckle_constant   ... on a constant map: one component, every border pixel joined
  fit_r7             pm_disparity_normals, r = 7, d_normals alone, max_diff 1, min_support 9

match and speckle_match are timed twice, interleaved with the other legs, so that a drift of the clocks shows as a difference
of the halves.  Event times include the launch gaps of the call's four launches and its memset.  Nothing is judged: the ratios
to fit_r7 and to the Match are reported.  Prints one JSON line; --record FILE writes the table and the tree's sha (--sha)
there.

--only LEG: that leg alone, 20 calls, no events (for a kernel trace of its own under a profiler)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from bench_rectify import event_timer

CAMERA = (1100.0, 1090.0, 640.3, 359.6, 0.12)
MAX_DIFF, MAX_SIZE = 1.0, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--record", default=None)
    ap.add_argument("--sha", default="unknown")
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    import pm_ctypes as pm
    import speckle_ref as SR
    import synth
    from fuzz_speckle import pattern
    rows, cols = 720, 1280
    res = {"steps": args.steps, "warmup": args.warmup}
    with pm.Engine(pm.default_params(0, patch=11, patchmatch_iters=8), max_rows=rows, max_cols=cols) as e:
        p = synth.make_pair(0, rows, cols)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        L, R, SL, SR_ = up(p["left"]), up(p["right"]), up(p["seed_l"]), up(p["seed_r"])
        DL = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
        DR = torch.zeros_like(DL)
        torch.cuda.synchronize()
        match = lambda: e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR_.data_ptr(), DL.data_ptr(),
                                       DR.data_ptr())
        match()
        e.synchronize()
        T, Rt = pm.speckle_constants()
        maps = {"match": DL.cpu().numpy(), "serpentine": pattern("serpentine", rows, cols, T, Rt, None)[0],
                "constant": pattern("constant", rows, cols, T, Rt, None)[0]}
        dev = {k: up(v) for k, v in maps.items()}
        out = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
        labels = torch.empty((rows, cols), dtype=torch.int32, device="cuda")
        sizes = torch.empty_like(labels)
        d_removed = torch.zeros(1, dtype=torch.int32, device="cuda")
        normals = torch.empty((rows, cols, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def speckle(k, everything=True):
            return lambda: e.filter_speckles(dev[k].data_ptr(), rows, cols, MAX_DIFF, MAX_SIZE, out.data_ptr(),
                                             labels.data_ptr() if everything else None, sizes.data_ptr() if everything else None,
                                             d_removed.data_ptr() if everything else None)

        legs = {
            "match": match,
            "speckle_match": speckle("match"),
            "speckle_match_out": speckle("match", False),
            "speckle_serpentine": speckle("serpentine"),
            "speckle_constant": speckle("constant"),
            "fit_r7": lambda: e.disparity_normals(CAMERA, dev["match"].data_ptr(), rows, cols, 7, 1.0, 9, normals.data_ptr()),
        }
        if args.only:
            for _ in range(20):
                legs[args.only]()
            e.synchronize()
            print(json.dumps({"only": args.only, "calls": 20}))
            return 0
        # what is timed is also right: each map's result against the definition, once
        res["maps"] = {}
        for k in maps:
            speckle(k)()
            e.synchronize()
            want = SR.filter_speckles(maps[k], MAX_DIFF, MAX_SIZE)
            same = (np.array_equal(labels.cpu().numpy(), want["labels"]) and np.array_equal(sizes.cpu().numpy(), want["sizes"])
                    and np.array_equal(out.cpu().numpy().view(np.uint32), want["out"].view(np.uint32))
                    and int(d_removed.cpu()[0]) == want["removed"])
            if not same:
                print("bench_speckle: the %s map differs from the definition" % k)
                return 1
            res["maps"][k] = {"valid_fraction": float((maps[k] > 0).mean()), "removed": want["removed"],
                              "components": int((want["labels"].ravel() == np.arange(rows * cols)).sum())}
        timed = event_timer(e, args.steps, args.warmup)
        order = ["match", "speckle_match"] + list(legs)
        res["legs"] = {}
        for name in order:
            res["legs"].setdefault(name, []).append(timed(legs[name]))
        e.synchronize()
    med = {k: float(np.median([r["median_ms"] for r in v])) for k, v in res["legs"].items()}
    res["median_ms"] = med
    res["speckle_match_over_fit_r7"] = med["speckle_match"] / med["fit_r7"]
    res["speckle_match_over_match"] = med["speckle_match"] / med["match"]
    res["serpentine_over_speckle_match"] = med["speckle_serpentine"] / med["speckle_match"]
    print(json.dumps(res))
    if args.record:
        with open(args.record, "w") as f:
            f.write("pm_filter_speckles beside the scalar Match() and pm_disparity_normals at r = 7 (tools/bench_speckle.py)\n")
            f.write("=" * 100 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            f.write("MI355X, one PM_MODE_SCALAR handle (11x11, 8 iterations, seeded, cross-check), 1280x720, HIP events on the\n"
                    "handle's stream, %d calls after %d warm-up calls per leg (match and speckle_match timed twice, interleaved).\n"
                    "max_diff %.1f, max_size %d.  Every timed map's labels, sizes, output and removed count equalled the definition.\n"
                    % (args.steps, args.warmup, MAX_DIFF, MAX_SIZE))
            for k, m in res["maps"].items():
                f.write("  map %-11s %.1f %% of its pixels > 0, %d components, %d pixels removed\n"
                        % (k, 100 * m["valid_fraction"], m["components"], m["removed"]))
            f.write("\nms:\n")
            for k, rs in res["legs"].items():
                for r in rs:
                    f.write("  %-19s median %.4f  min %.4f  max %.4f\n" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
            f.write("  speckle_match / fit_r7 = %.2f;  speckle_match / match = %.3f;  speckle_serpentine / speckle_match = %.2f\n"
                    % (res["speckle_match_over_fit_r7"], res["speckle_match_over_match"], res["serpentine_over_speckle_match"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
