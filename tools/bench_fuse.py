#!/usr/bin/env python3
"""Times pm_fuse_disparity beside its nearest stages, pm_filter_consistency (whose gather is a subset of its own) and
pm_reproject_disparity (whose splat launch its fill runs once per source), on the same handle, maps and run, and reports what
the fusion does to a map.

Timing.  The map and the sources are tools/bench_consistency.py's: a scalar pm_match_device (8 iterations, the default 11x11
window) of the benchmark's synthetic 1280x720 pair, tiled to 4096x2160 for the larger size; source k is that map carried k + 1
frames back by pm_reproject_disparity (close_radius 1) under a yaw of k + 1 degrees and (k + 1) x (1 cm sideways, 5 cm along
the axis).  8 % of the current map's pixels are then zeroed, so that the fill has work.  Legs, each timed with HIP events on the
handle's stream around every call, median (min / max) over --steps calls after --warmup, every leg TWICE, interleaved, so that
a drift of the clocks shows as a difference of the halves; n = 1 and 4, radius 1:

  cons_nN       pm_filter_consistency, all outputs                         a 16-byte memset, one launch, an 8-byte copy
  fuse_nN       pm_fuse_disparity, the fill off, all outputs, no weights   a 16-byte memset, one launch, a 16-byte copy
  fuse_nN_w     ... with a weight plane for the map and for every source
  fill_nN       pm_fuse_disparity with fill_min_sources = 1                a memset of n maps, two launches, a 16-byte copy
  splat_nN      N calls of pm_reproject_disparity with d_seed_l alone      per call: a memset of two maps, the splat launch and
                                                                           its close + count launch (the C ABI has no smaller
                                                                           unit that holds the splat launch)

Every leg passes device counts and no host counts: nothing synchronises inside the timed window.  max_diff 1, min_consistent 1,
max_conflicts 0.  Nothing is gated: the exit status is 0 either way.

Quality (reported, not asserted).  The benchmark's synthetic 1280x720 pair matched three times (scalar, 8 iterations) with
different noise_seed; map 1 fused against maps 2 and 3 under the identity motion, max_diff 1, radius 1, min_consistent 1,
max_conflicts 0, fill_min_sources 2, fill_max_diff 1: the mean |error| against the ground truth over the fused pixels before
and after, and the filled pixels with the share of them within 1 px of the ground truth.

Prints one JSON line; --record FILE writes the times, the ratios and the quality table there, stamped with --sha.
--no-quality / --no-timing skip a half."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from bench_cloud import SIZES, camera_for
from bench_consistency import SEEDS, frame_motion, match
from bench_rectify import event_timer
from fuzz_reproject import IDENTITY

SOURCES = (1, 4)
RADIUS = 1


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
    res = {"steps": args.steps, "warmup": args.warmup, "radius": RADIUS, "sizes": {}}
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
                full_np = np.tile(match_map, (-(-rows // 720), -(-cols // 1280)))[:rows, :cols]
                full = torch.from_numpy(np.ascontiguousarray(full_np)).cuda()
                disp_np = full_np.copy()
                disp_np[np.random.default_rng(5).random((rows, cols)) < 0.08] = 0.0
                disp = torch.from_numpy(disp_np).cuda()
                src = torch.zeros((n_max, rows, cols), dtype=torch.float32, device="cuda")
                wts = torch.rand((n_max + 1, rows, cols), dtype=torch.float32, device="cuda") + 0.5
                out = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
                seed = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
                spr = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
                cls = torch.empty((rows, cols), dtype=torch.int16, device="cuda")
                cnt = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
                flg = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
                d_cnt = torch.zeros((4,), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                motions = [frame_motion(k) for k in range(n_max)]
                seeded = [e.reproject_disparity(cam, motions[k], full.data_ptr(), rows, cols, d_seed_l=src[k].data_ptr(),
                                                want_counts=True)[0] / (rows * cols) for k in range(n_max)]
                ptrs = [src[k].data_ptr() for k in range(n_max)]

                def consistency(n, host=False):
                    return e.filter_consistency(cam, disp.data_ptr(), ptrs[:n], motions[:n], rows, cols, max_diff=1.0, radius=RADIUS,
                                                min_consistent=1, max_conflicts=0, d_out=out.data_ptr(), d_classes=cls.data_ptr(),
                                                d_residual=spr.data_ptr(), d_counts=d_cnt.data_ptr(), want_counts=host)

                def fuse(n, fill, weighted=False, host=False):
                    return e.fuse_disparity(cam, disp.data_ptr(), ptrs[:n], motions[:n], rows, cols, max_diff=1.0, radius=RADIUS,
                                            min_consistent=1, max_conflicts=0, fill_min_sources=fill, fill_max_diff=1.0,
                                            d_weight=wts[n_max].data_ptr() if weighted else None,
                                            d_source_weights=[wts[k].data_ptr() for k in range(n)] if weighted else None,
                                            d_out=out.data_ptr(), d_count=cnt.data_ptr(), d_spread=spr.data_ptr(),
                                            d_flags=flg.data_ptr(), d_counts=d_cnt.data_ptr(), want_counts=host)

                def splats(n):
                    for k in range(n):
                        e.reproject_disparity(cam, motions[k], src[k].data_ptr(), rows, cols, close_radius=0, d_seed_l=seed.data_ptr())

                legs, counts = {}, {}
                for n in SOURCES:
                    consistency(n, host=True)  # the scratch, outside the timing
                    counts["fuse_n%d" % n] = fuse(n, 0, host=True)
                    counts["fill_n%d" % n] = fuse(n, 1, host=True)
                    legs["cons_n%d" % n] = (lambda n=n: consistency(n))
                    legs["fuse_n%d" % n] = (lambda n=n: fuse(n, 0))
                    legs["fuse_n%d_w" % n] = (lambda n=n: fuse(n, 0, True))
                    legs["fill_n%d" % n] = (lambda n=n: fuse(n, 1))
                    legs["splat_n%d" % n] = (lambda n=n: splats(n))
                o = {"pixels": rows * cols, "valid_in": float((disp_np > 0).mean()), "source_share": seeded,
                     "counts": {k: list(v) for k, v in counts.items()}, "legs": {}}
                for name in list(legs) + list(legs):  # every leg twice, interleaved
                    o["legs"].setdefault(name, []).append(timed(legs[name]))
                e.synchronize()
                o["median_ms"] = {k: float(np.median([r["median_ms"] for r in v])) for k, v in o["legs"].items()}
                m = o["median_ms"]
                o["ratio"] = {}
                for n in SOURCES:
                    o["ratio"]["fuse_n%d / cons_n%d" % (n, n)] = m["fuse_n%d" % n] / m["cons_n%d" % n]
                    o["ratio"]["fuse_n%d_w / cons_n%d" % (n, n)] = m["fuse_n%d_w" % n] / m["cons_n%d" % n]
                    o["ratio"]["fill_n%d / (fuse_n%d + splat_n%d)" % (n, n, n)] = m["fill_n%d" % n] / (m["fuse_n%d" % n] + m["splat_n%d" % n])
                res["sizes"]["%dx%d" % (cols, rows)] = o

    if not args.no_quality:
        rows, cols = 720, 1280
        cam = camera_for(rows)
        maps += [match(pm, torch, pair, s) for s in SEEDS[1:]]
        out = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
        flg = torch.zeros((rows, cols), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        gt = pair["gt"]
        with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
            n = e.fuse_disparity(cam, maps[0].data_ptr(), [maps[1].data_ptr(), maps[2].data_ptr()], [IDENTITY] * 2, rows, cols,
                                 max_diff=1.0, radius=1, min_consistent=1, max_conflicts=0, fill_min_sources=2, fill_max_diff=1.0,
                                 d_out=out.data_ptr(), d_flags=flg.data_ptr(), want_counts=True)
            e.synchronize()
        got, flags = out.cpu().numpy(), flg.cpu().numpy()
        fused, filled = (flags & pm.PM_FUSE_FUSED) != 0, (flags & pm.PM_FUSE_FILLED) != 0
        res["quality"] = {
            "counts": list(n),
            "fused_mean_abs_error_before": float(np.abs(match_map - gt)[fused].mean()) if fused.any() else 0.0,
            "fused_mean_abs_error_after": float(np.abs(got - gt)[fused].mean()) if fused.any() else 0.0,
            "filled_within_1px": float((np.abs(got - gt)[filled] <= 1.0).mean()) if filled.any() else 0.0,
            "holes_before": int((match_map <= 0).sum()),
        }

    print(json.dumps(res))
    if args.record:
        with open(args.record, "w") as f:
            f.write("pm_fuse_disparity beside pm_filter_consistency and pm_reproject_disparity (tools/bench_fuse.py)\n" + "=" * 100 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            if res["sizes"]:
                f.write("MI355X, one handle, HIP events on the handle's stream, same run, %d calls after %d warm-up calls per leg,\n"
                        "every leg timed twice, interleaved.  The map: a real scalar match (8 iterations) of the benchmark's synthetic\n"
                        "1280x720 pair, %.1f %% of its pixels > 0, tiled to the larger size, 8 %% of its pixels then zeroed.  Source k: the\n"
                        "map carried k + 1 frames back by pm_reproject_disparity (yaw k + 1 degrees, t = (k + 1) x (0.01, 0, -0.05) m,\n"
                        "close_radius 1).  radius %d, max_diff 1, min_consistent 1, max_conflicts 0, all outputs, device counts.\n\n"
                        % (args.steps, args.warmup, 100 * res["match_valid_fraction"], RADIUS))
                for size, o in res["sizes"].items():
                    f.write("%s: %d pixels, %.1f %% > 0 in; sources > 0: %s %%; ms:\n"
                            % (size, o["pixels"], 100 * o["valid_in"], " / ".join("%.1f" % (100 * v) for v in o["source_share"])))
                    for k, rs in o["legs"].items():
                        for r in rs:
                            f.write("  %-12s median %.4f  min %.4f  max %.4f\n" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
                    for k, v in o["ratio"].items():
                        f.write("  %s = %.3f\n" % (k, v))
                    for k, v in o["counts"].items():
                        f.write("  %s: valid %d, kept %d, fused %d, filled %d\n" % (k, *v))
                    f.write("\n")
                f.write("Event times include the launch gaps; at 1280x720 they weigh.\n\n")
            if "quality" in res:
                q = res["quality"]
                f.write("Quality on the 1280x720 pair (reported, not asserted): map 1 of three scalar matches (8 iterations) that differ in\n"
                        "noise_seed (%s), fused against maps 2 and 3 under the identity motion; max_diff 1, radius 1, min_consistent 1,\n"
                        "max_conflicts 0, fill_min_sources 2, fill_max_diff 1.\n\n" % ", ".join(str(s) for s in SEEDS))
                f.write("  valid %d, kept %d, fused %d, filled %d of %d pixels without a value\n" % (*q["counts"], q["holes_before"]))
                f.write("  mean |error| against the ground truth over the fused pixels: %.4f before, %.4f after\n"
                        % (q["fused_mean_abs_error_before"], q["fused_mean_abs_error_after"]))
                f.write("  filled pixels within 1 px of the ground truth: %.2f %%\n" % (100 * q["filled_within_1px"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
