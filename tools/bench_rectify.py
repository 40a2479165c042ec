#!/usr/bin/env python3
"""Times the rectification of a raw stereo pair on the device (a record, not a gate).

  (a) pm_rectify_u8 of the left and of the right image of a rows x cols pair (two launches, no mask), views from
      pm_stereo_rectify of a EuRoC-like calibration (radial-tangential distortion, a small relative rotation).
  (b) the same with the validity masks.
  (c) pm_stereo_ready of ONE rows x cols BGR image on the same run, the other per-frame stage in front of Match(), for
      scale.

HIP events on the handle's stream around every call; median (and min / max) over --steps calls after --warmup.
Prints one JSON line; --record FILE also writes the figures there, with the tree's sha when --sha gives one.
--only a | b | c restricts the run (e.g. for a kernel trace of (a) alone)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
import numpy as np


def calibration(rows, cols):
    """A EuRoC-like pair scaled to the image size: about 458 px focal length at 752 px width."""
    f = 458.0 * cols / 752.0
    cam1 = (f, 0.997 * f, 0.49 * cols, 0.52 * rows, -0.28, 0.07, 2e-4, 2e-5, 0.0)
    cam2 = (0.998 * f, 0.995 * f, 0.51 * cols, 0.53 * rows, -0.283, 0.074, -1e-4, -3.5e-5, 0.0)

    def rot(axis, deg):
        c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        R = np.eye(3)
        R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
        return R

    return cam1, cam2, rot(2, 0.3) @ rot(1, 0.8) @ rot(0, 0.5), np.array([-0.11, 0.0004, -0.0006])


def event_timer(engine, steps, warmup):
    """-> timed(fn): fn `warmup` times, then HIP events on the handle's stream around each of `steps` calls; ms."""
    import torch
    stream = torch.cuda.ExternalStream(engine.stream())

    def timed(fn):
        for _ in range(warmup):
            fn()
        engine.synchronize()
        ms = []
        for _ in range(steps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            fn()
            t1.record(stream)
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}

    return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=720)
    ap.add_argument("--cols", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=("a", "b", "c"), default=None)
    ap.add_argument("--record", default=None)
    ap.add_argument("--sha", default="unknown")
    args = ap.parse_args()
    import torch
    import pm_ctypes as pm
    rows, cols = args.rows, args.cols
    v1, v2, baseline = pm.stereo_rectify(*calibration(rows, cols))
    g = torch.Generator(device="cuda").manual_seed(1)
    raw = torch.randint(0, 256, (2, rows, cols), device="cuda", generator=g, dtype=torch.uint8)
    bgr = torch.randint(0, 256, (rows, cols, 3), device="cuda", generator=g, dtype=torch.uint8)
    out = torch.empty_like(raw)
    mask = torch.empty_like(raw)
    gray = torch.empty((rows, cols), device="cuda", dtype=torch.uint8)
    torch.cuda.synchronize()
    res = {"rows": rows, "cols": cols, "steps": args.steps, "baseline": baseline,
           "pair_bytes_read_and_written": 4 * rows * cols}
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        timed = event_timer(e, args.steps, args.warmup)

        def pair(with_mask):
            for i, v in enumerate((v1, v2)):
                e.rectify_u8(v, raw[i].data_ptr(), 1, rows, cols, 0, rows, cols, 0, out[i].data_ptr(),
                             mask[i].data_ptr() if with_mask else None)

        if args.only in (None, "a"):
            res["a_rectify_pair"] = timed(lambda: pair(False))
        if args.only in (None, "b"):
            res["b_rectify_pair_with_masks"] = timed(lambda: pair(True))
        if args.only in (None, "c"):
            res["c_stereo_ready_one_image"] = timed(lambda: e.stereo_ready(bgr.data_ptr(), rows, cols, None, gray.data_ptr()))
        e.synchronize()
        res["valid_fraction_left"] = float((mask[0] == 255).float().mean()) if args.only in (None, "b") else None
    print(json.dumps(res))
    if args.record:
        with open(args.record, "w") as f:
            f.write("Rectification of a raw stereo pair on the device (tools/bench_rectify.py)\n")
            f.write("=" * 72 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            f.write("MI355X, %dx%d pair, HIP events on the handle's stream, %d calls after %d warm-up calls, ms:\n\n" %
                    (cols, rows, args.steps, args.warmup))
            for key in ("a_rectify_pair", "b_rectify_pair_with_masks", "c_stereo_ready_one_image"):
                if key in res:
                    f.write("  %-28s median %.4f  min %.4f  max %.4f\n" % (key, res[key]["median_ms"], res[key]["min_ms"],
                                                                        res[key]["max_ms"]))
            f.write("\n(a), (b): two launches of k_rectify (left, right), each event pair spans both; (c): pm_stereo_ready of\n"
                    "one BGR image of the same size on the same run, for scale.  Event times include the launch gaps.\n")


if __name__ == "__main__":
    main()
