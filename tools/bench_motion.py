#!/usr/bin/env python3
"""Times pm_track_features and pm_estimate_motion at 1280x720 (cell 16, p = 5, s = 12) beside one Match() of the same size, on
the same run.

The old frame is the left image of the benchmark's synthetic pair with the left map of a scalar pm_match_device (8 iterations)
of that pair; the new frame is that scene seen after a yaw of 0.2 degrees and 2 cm sideways: every pixel of the old image
carried by pm_reproject_disparity's arithmetic (tests/motion_ref.py: predict) to where it lands, nearest pixel, holes left at
the old value -- a stand-in that gives the matcher real work, not an accuracy test (tests/test_motion.py has that).

Legs, each timed with HIP events on the handle's stream around every call, median (min / max) over --steps calls after
--warmup, every leg TWICE, interleaved:

  count      pm_track_features with capacity 0, d_count alone       k_track_select + k_track_compact
  track      pm_track_features into a device buffer, d_count alone  k_track_select + k_track_compact + k_track_match
  match      one scalar pm_match_device, 8 iterations               the whole Match() of the pair

k_track_match is reported as track - count.  The whole pm_estimate_motion call (the three launches, the download of the count
and of the records, the solve on the host; it synchronises) is timed with the host's clock around the call.  Nothing is gated:
the exit status is 0 either way.  Prints one JSON line; --record FILE writes the table there, stamped with --sha."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import motion_ref as MR
from bench_cloud import camera_for
from bench_consistency import SEEDS, match
from bench_rectify import event_timer
from fuzz_reproject import rotation

TRACK = dict(cell=16, patch_radius=5, search_radius=12, min_score=1)
SOLVE = dict(iterations=10, huber_px=1.0, epsilon=1e-9, inlier_px=1.0, min_inliers=30)


def moved(image, disp, cam, motion):
    """The old image forward-warped through `motion` by the nearest pixel, far surfaces first; holes keep the old value."""
    rows, cols = image.shape
    y, x = np.mgrid[0:rows, 0:cols]
    ok = np.isfinite(disp) & (disp > 0)
    X, Y, Z = MR.point(cam, x, y, np.where(ok, disp, np.float32(1)))
    Xn, Yn, Zn = MR.transform(motion[0], motion[1], X, Y, Z)
    with np.errstate(all="ignore"):
        u, v = np.rint(cam[0] * Xn / Zn + cam[2]), np.rint(cam[1] * Yn / Zn + cam[3])
    ok &= (Zn > 0) & (u >= 0) & (u < cols) & (v >= 0) & (v < rows)
    order = np.argsort(-Zn[ok], kind="stable")
    out = image.copy()
    out[v[ok].astype(np.int64)[order], u[ok].astype(np.int64)[order]] = image[ok][order]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--record", default=None)
    ap.add_argument("--sha", default="unknown")
    args = ap.parse_args()
    import torch
    import pm_ctypes as pm
    import synth
    rows, cols = 720, 1280
    cam = camera_for(rows)
    pair = synth.make_pair(0, rows, cols)
    d_disp = match(pm, torch, pair, SEEDS[0])
    disp = d_disp.cpu().numpy()
    truth = (rotation((0, 1, 0), 0.2).ravel(), np.array([0.02, 0.0, 0.0]))
    old = np.ascontiguousarray(pair["left"])
    new = moved(old, disp, cam, truth)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_old, d_new = up(old), up(new)
    L, R, SL, SR = up(pair["left"]), up(pair["right"]), up(pair["seed_l"]), up(pair["seed_r"])
    DL, DR = torch.zeros((rows, cols), dtype=torch.float32, device="cuda"), torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    cells = -(-rows // TRACK["cell"]) * -(-cols // TRACK["cell"])
    rec = torch.zeros(32 * cells, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res = {"steps": args.steps, "warmup": args.warmup, "size": "%dx%d" % (cols, rows), "track_options": TRACK, "solve_options": SOLVE,
           "cells": cells, "legs": {}}
    with pm.Engine(pm.default_params(0, patchmatch_iters=8), max_rows=rows, max_cols=cols) as e:
        timed = event_timer(e, args.steps, args.warmup)
        ptrs = (d_old.data_ptr(), d_disp.data_ptr(), d_new.data_ptr())
        res["features"] = e.track_features(cam, *ptrs, rows, cols, capacity=cells, d_tracks=rec.data_ptr(), want_count=True, **TRACK)
        tracks = rec.cpu().numpy().view(MR.TRACK)[:res["features"]]
        res["ok_tracks"] = int(MR.ok_tracks(tracks).sum())
        legs = {
            "count": lambda: e.track_features(cam, *ptrs, rows, cols, capacity=0, d_count=cnt.data_ptr(), **TRACK),
            "track": lambda: e.track_features(cam, *ptrs, rows, cols, capacity=cells, d_tracks=rec.data_ptr(), d_count=cnt.data_ptr(), **TRACK),
            "match": lambda: e.match_device(1, L.data_ptr(), R.data_ptr(), rows, cols, SL.data_ptr(), SR.data_ptr(), DL.data_ptr(), DR.data_ptr()),
        }
        for name in list(legs) + list(legs):  # every leg twice, interleaved
            res["legs"].setdefault(name, []).append(timed(legs[name]))
        e.synchronize()
        whole = []
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            Rm, tm, info = e.estimate_motion(cam, *ptrs, rows, cols, None, TRACK, SOLVE)
            if k >= args.warmup:
                whole.append(1e3 * (time.perf_counter() - t0))
    res["estimate_ms"] = {"median_ms": float(np.median(whole)), "min_ms": float(min(whole)), "max_ms": float(max(whole))}
    res["info"] = info
    res["rotation_error_deg"] = float(np.degrees(2 * np.arcsin(min(np.linalg.norm(Rm - truth[0]) / (2 * np.sqrt(2)), 1.0))))
    res["translation_error_m"] = float(np.linalg.norm(tm - truth[1]))
    m = {k: float(np.median([r["median_ms"] for r in v])) for k, v in res["legs"].items()}
    m["k_track_match (track - count)"] = m["track"] - m["count"]
    res["median_ms"] = m
    print(json.dumps(res))
    if args.record:
        with open(args.record, "w") as f:
            f.write("pm_track_features and pm_estimate_motion beside one Match() (tools/bench_motion.py)\n" + "=" * 100 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            f.write("MI355X, one handle, %s, cell %d, p = %d, s = %d: %d cells, %d features, %d OK tracks.  HIP events on the handle's\n"
                    "stream, same run, %d calls after %d warm-up calls per leg, every leg timed twice, interleaved; ms:\n\n"
                    % (res["size"], TRACK["cell"], TRACK["patch_radius"], TRACK["search_radius"], cells, res["features"], res["ok_tracks"],
                       args.steps, args.warmup))
            for k, rs in res["legs"].items():
                for r in rs:
                    f.write("  %-8s median %.4f  min %.4f  max %.4f\n" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
            f.write("\n  count: k_track_select + k_track_compact;  track: those and k_track_match;  match: one scalar Match(), 8 iterations\n")
            f.write("  k_track_match = track - count = %.4f ms\n\n" % m["k_track_match (track - count)"])
            w = res["estimate_ms"]
            f.write("pm_estimate_motion, the whole call with the download and the solve (%d iterations made, %d inliers of %d tracks),\n"
                    "host clock around the call: median %.4f  min %.4f  max %.4f ms\n"
                    % (info["iterations"], info["n_inliers"], info["n_tracks"], w["median_ms"], w["min_ms"], w["max_ms"]))
            f.write("against the motion the new frame was warped with: rotation error %.4f deg, translation error %.4f m (valid %d)\n\n"
                    % (res["rotation_error_deg"], res["translation_error_m"], info["valid"]))
            f.write("Reported, not asserted.  Event times include the launch gaps.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
