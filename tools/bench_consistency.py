#!/usr/bin/env python3
"""Times pm_filter_consistency beside its yardstick, pm_backproject, on the same handle, map and run, and reports what the
filter does to a map.

Timing.  The map is a REAL match's, as in tools/bench_reproject.py: a scalar pm_match_device (8 iterations, the default 11x11
window) of the benchmark's synthetic 1280x720 pair, standard seeds; at 4096x2160 the same map is tiled to the size.  Source k
(k = 0 .. n - 1) is that map carried k + 1 frames back by pm_reproject_disparity (close_radius 1) under the motion
tools/bench_reproject.py uses per frame -- a yaw of k + 1 degrees, (k + 1) x (1 cm sideways, 5 cm along the axis) -- each in a
buffer of its own.  Legs, each timed with HIP events on the handle's stream around every call, median (min / max) over --steps
calls after --warmup, every leg TWICE, interleaved, so that a drift of the clocks shows as a difference of the halves:

  backproject      pm_backproject                                              one launch
  n1_r0, n1_r1     pm_filter_consistency, 1 source, radius 0 / 1, all outputs  a 16-byte memset, one launch, an 8-byte copy
  n4_r0, n4_r1     ... 4 sources

Every leg passes device counts and no host counts: nothing synchronises inside the timed window.  max_diff 1, min_consistent 1,
max_conflicts 0.

The byte model (radius 0):  B_consistency = 4 + 4 n read + 10 written per pixel;  B_backproject = 4 + 12 = 16.  An HBM-bound
kernel would stay within  t_consistency / t_backproject <= 1.5 * B_consistency / 16  (1.5: gathers that do not fill their cache
lines): 1.69 for n = 1, 2.81 for n = 4.  Whether bytes bind at all is what this tool records: the kernel also does 3 + 3 n
binary64 divisions per pixel.  The ratio is REPORTED, not a gate: the exit status is 0 either way.

Quality (reported, not asserted).  The benchmark's synthetic 1280x720 pair matched three times (scalar, 8 iterations) with
different noise_seed; map 1 filtered against maps 2 and 3 under the identity motion, max_diff 1, radius 1, max_conflicts 0:
the share of valid pixels kept for min_consistent 1 and 2, and the share of the valid (kept) pixels within 1 px of the ground
truth before and after.

Prints one JSON line; --record FILE writes the model, the times, the ratios and the quality table there, stamped with --sha.
--no-quality / --no-timing skip a half."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from bench_cloud import SIZES, camera_for
from bench_rectify import event_timer
from fuzz_reproject import IDENTITY, rotation

FACTOR = 1.5
BYTES_BACKPROJECT = 16
SOURCES = (1, 4)
RADII = (0, 1)
SEEDS = (123, 1123, 2123)


def frame_motion(k):
    """The camera k + 1 frames back: tools/bench_reproject.py's per-frame motion, k + 1 times as far."""
    return (rotation((0, 1, 0), 1.0 * (k + 1)).ravel(), np.array([0.01, 0.0, -0.05]) * (k + 1))


def bytes_consistency(n):
    return 4 + 4 * n + 10


def match(pm, torch, pair, noise_seed):
    """One scalar match (8 iterations) of the pair with that noise_seed -> the left map as a device tensor."""
    rows, cols = pair["left"].shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    L, R, SL, SR = up(pair["left"]), up(pair["right"]), up(pair["seed_l"]), up(pair["seed_r"])
    DL = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    DR = torch.zeros_like(DL)
    torch.cuda.synchronize()
    with pm.Engine(pm.default_params(0, patchmatch_iters=8, noise_seed=noise_seed), max_rows=rows, max_cols=cols) as e:
        e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), DL.data_ptr(), DR.data_ptr())
        e.synchronize()
    return DL


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--record", default=None)
    ap.add_argument("--sha", default="unknown")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--no-timing", action="store_true")
    args = ap.parse_args()
    import torch
    import pm_ctypes as pm
    import synth
    big = "%dx%d" % (max(c for _, c in SIZES), max(r for r, _ in SIZES))
    res = {"steps": args.steps, "warmup": args.warmup, "factor": FACTOR, "sizes": {}}
    pair = synth.make_pair(0, 720, 1280)
    maps = [match(pm, torch, pair, SEEDS[0])]
    match_map = maps[0].cpu().numpy()
    res["match_valid_fraction"] = float((match_map > 0).mean())

    if not args.no_timing:
        n_max = max(SOURCES)
        with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
            timed = event_timer(e, args.steps, args.warmup)
            for rows, cols in SIZES:
                cam = camera_for(rows)
                disp_np = np.tile(match_map, (-(-rows // 720), -(-cols // 1280)))[:rows, :cols]
                disp = torch.from_numpy(np.ascontiguousarray(disp_np)).cuda()
                xyz = torch.empty((rows, cols, 3), dtype=torch.float32, device="cuda")
                src = torch.zeros((n_max, rows, cols), dtype=torch.float32, device="cuda")
                out = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
                cls = torch.empty((rows, cols), dtype=torch.int16, device="cuda")
                rsd = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
                d_cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                motions = [frame_motion(k) for k in range(n_max)]
                seeded = [e.reproject_disparity(cam, motions[k], disp.data_ptr(), rows, cols, d_seed_l=src[k].data_ptr(),
                                                want_counts=True)[0] / (rows * cols) for k in range(n_max)]

                def consistency(n, radius, host=False):
                    return e.filter_consistency(cam, disp.data_ptr(), [src[k].data_ptr() for k in range(n)], motions[:n], rows, cols,
                                                max_diff=1.0, radius=radius, min_consistent=1, max_conflicts=0,
                                                d_out=out.data_ptr(), d_classes=cls.data_ptr(), d_residual=rsd.data_ptr(),
                                                d_counts=d_cnt.data_ptr(), want_counts=host)

                legs = {"backproject": lambda: e.backproject(cam, disp.data_ptr(), rows, cols, xyz.data_ptr())}
                counts = {}
                for n in SOURCES:
                    for radius in RADII:
                        name = "n%d_r%d" % (n, radius)
                        counts[name] = consistency(n, radius, host=True)  # and the scratch, outside the timing
                        legs[name] = (lambda n=n, radius=radius: consistency(n, radius))
                o = {"pixels": rows * cols, "valid_in": float((disp_np > 0).mean()), "source_share": seeded,
                     "kept_share": {k: v[1] / max(v[0], 1) for k, v in counts.items()}, "legs": {}}
                for name in list(legs) + list(legs):  # every leg twice, interleaved
                    o["legs"].setdefault(name, []).append(timed(legs[name]))
                e.synchronize()
                o["median_ms"] = {k: float(np.median([r["median_ms"] for r in v])) for k, v in o["legs"].items()}
                o["ratio"] = {k: v / o["median_ms"]["backproject"] for k, v in o["median_ms"].items() if k != "backproject"}
                o["budget"] = {"n%d_r0" % n: FACTOR * bytes_consistency(n) / BYTES_BACKPROJECT for n in SOURCES}
                o["gb_per_s"] = {"backproject": BYTES_BACKPROJECT * rows * cols / (o["median_ms"]["backproject"] * 1e-3) / 1e9}
                for n in SOURCES:
                    o["gb_per_s"]["n%d_r0" % n] = bytes_consistency(n) * rows * cols / (o["median_ms"]["n%d_r0" % n] * 1e-3) / 1e9
                res["sizes"]["%dx%d" % (cols, rows)] = o
        res["within_byte_budget"] = {k: bool(res["sizes"][big]["ratio"][k] <= v) for k, v in res["sizes"][big]["budget"].items()}

    if not args.no_quality:
        rows, cols = 720, 1280
        cam = camera_for(rows)
        maps += [match(pm, torch, pair, s) for s in SEEDS[1:]]
        out = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        gt = pair["gt"]

        def quality(d):
            ok = d > 0
            return {"valid": float(ok.mean()), "within_1px_of_valid": float((np.abs(d - gt)[ok] <= 1.0).mean()) if ok.any() else 0.0}

        res["quality"] = {"before": quality(match_map), "after": {}}
        with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
            for mc in (1, 2):
                n = e.filter_consistency(cam, maps[0].data_ptr(), [maps[1].data_ptr(), maps[2].data_ptr()], [IDENTITY] * 2, rows, cols,
                                         max_diff=1.0, radius=1, min_consistent=mc, max_conflicts=0, d_out=out.data_ptr(),
                                         want_counts=True)
                e.synchronize()
                q = quality(out.cpu().numpy())
                q["kept_of_valid"] = n[1] / max(n[0], 1)
                res["quality"]["after"][str(mc)] = q

    print(json.dumps(res))
    if args.record:
        with open(args.record, "w") as f:
            f.write("pm_filter_consistency beside pm_backproject (tools/bench_consistency.py)\n" + "=" * 100 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            if "sizes" in res and res["sizes"]:
                f.write("MI355X, one handle, HIP events on the handle's stream, same run, %d calls after %d warm-up calls per leg,\n"
                        "every leg timed twice, interleaved.  The map: a real scalar match (8 iterations) of the benchmark's synthetic\n"
                        "1280x720 pair, %.1f %% of its pixels > 0; tiled to the larger size.  Source k: that map carried k + 1 frames back\n"
                        "by pm_reproject_disparity (yaw k + 1 degrees, t = (k + 1) x (0.01, 0, -0.05) m, close_radius 1).  All outputs\n"
                        "(d_out, d_classes, d_residual, d_counts), max_diff 1, min_consistent 1, max_conflicts 0.\n\n"
                        % (args.steps, args.warmup, 100 * res["match_valid_fraction"]))
                f.write("Byte model (radius 0): 4 + 4 n read + 10 written per pixel against pm_backproject's 4 + 12 = 16; an HBM-bound kernel\n"
                        "would stay within %.1f x that ratio.  Reported, not a gate.\n\n" % FACTOR)
                for size, o in res["sizes"].items():
                    f.write("%s: %d pixels, %.1f %% > 0 in; sources > 0: %s %%; ms:\n"
                            % (size, o["pixels"], 100 * o["valid_in"], " / ".join("%.1f" % (100 * v) for v in o["source_share"])))
                    for k, rs in o["legs"].items():
                        for r in rs:
                            f.write("  %-12s median %.4f  min %.4f  max %.4f\n" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
                    for k, v in o["ratio"].items():
                        note = ""
                        if k in o["budget"]:
                            note = "; byte budget %.2f -> %s; %.0f GB/s of the model's bytes" % (
                                o["budget"][k], "within" if v <= o["budget"][k] else "ABOVE by %.2f" % (v - o["budget"][k]), o["gb_per_s"][k])
                        f.write("  t_%s %.4f / t_backproject %.4f = %.3f; kept %.1f %% of the valid pixels%s\n"
                                % (k, o["median_ms"][k], o["median_ms"]["backproject"], v, 100 * o["kept_share"][k], note))
                    f.write("  pm_backproject: %.0f GB/s of its 16 bytes per pixel\n\n" % o["gb_per_s"]["backproject"])
                f.write("Event times include the launch gaps (a memset, a launch and a copy against one launch); at 1280x720 they weigh.\n\n")
            if "quality" in res:
                q = res["quality"]
                f.write("Quality on the 1280x720 pair (reported, not asserted): map 1 of three scalar matches (8 iterations) that differ in\n"
                        "noise_seed (%s), filtered against maps 2 and 3 under the identity motion; max_diff 1, radius 1, max_conflicts 0.\n\n"
                        % ", ".join(str(s) for s in SEEDS))
                f.write("  %-22s  valid of all pixels   kept of the valid   within 1 px of the ground truth (of the valid left)\n" % "")
                f.write("  %-22s  %17.1f %%  %17s  %10.2f %%\n" % ("before", 100 * q["before"]["valid"], "", 100 * q["before"]["within_1px_of_valid"]))
                for mc, v in q["after"].items():
                    f.write("  %-22s  %17.1f %%  %15.2f %%  %10.2f %%\n" % ("min_consistent %s" % mc, 100 * v["valid"], 100 * v["kept_of_valid"],
                                                                       100 * v["within_1px_of_valid"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
