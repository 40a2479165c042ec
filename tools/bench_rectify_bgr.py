#!/usr/bin/env python3
"""Times pm_rectify_bgr8 against the three pm_rectify_u8 launches it replaces.

  gray  pm_rectify_u8 of ONE rows x cols gray image (existing code, the baseline)
  bgr   pm_rectify_bgr8 of ONE rows x cols interleaved BGR image, the 8-bit output alone
  bgr_float / bgr_all: the same with the float image instead of / next to the 8-bit one and the mask (for the record)

Same run, same handle, same view: the left view of tools/bench_rectify.py's EuRoC-like calibration (radial-tangential
distortion) and its timing loop: HIP events on the handle's stream around every call, median (and min / max) over
--steps calls after --warmup.  The criterion: the bgr median is below 3 x the gray median -- three gray launches are
what the kernel replaces.  Prints one JSON line; --record FILE also writes the figures there, with the tree's sha when --sha gives one.
Exit status 1 when the criterion is missed."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from bench_rectify import calibration, event_timer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=720)
    ap.add_argument("--cols", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--record", default=None)
    ap.add_argument("--sha", default="unknown")
    args = ap.parse_args()
    assert args.steps >= 20
    import torch
    import pm_ctypes as pm
    rows, cols = args.rows, args.cols
    view, _, _ = pm.stereo_rectify(*calibration(rows, cols))
    g = torch.Generator(device="cuda").manual_seed(1)
    gray = torch.randint(0, 256, (rows, cols), device="cuda", generator=g, dtype=torch.uint8)
    bgr = torch.randint(0, 256, (rows, cols, 3), device="cuda", generator=g, dtype=torch.uint8)
    gray_out, bgr_out = torch.empty_like(gray), torch.empty_like(bgr)
    bgr_f = torch.empty((rows, cols, 3), device="cuda", dtype=torch.float32)
    mask = torch.empty_like(gray)
    torch.cuda.synchronize()
    res = {"rows": rows, "cols": cols, "steps": args.steps, "warmup": args.warmup}
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        timed = event_timer(e, args.steps, args.warmup)

        def run_bgr(d8, df, dm):
            e.rectify_bgr8(view, bgr.data_ptr(), 1, rows, cols, 0, rows, cols, 0, d8, df, dm)

        legs = (("gray", lambda: e.rectify_u8(view, gray.data_ptr(), 1, rows, cols, 0, rows, cols, 0, gray_out.data_ptr())),
                ("bgr", lambda: run_bgr(bgr_out.data_ptr(), None, None)),
                ("bgr_float", lambda: run_bgr(None, bgr_f.data_ptr(), None)),
                ("bgr_all", lambda: run_bgr(bgr_out.data_ptr(), bgr_f.data_ptr(), mask.data_ptr())))
        # gray and bgr twice, interleaved, so that a drift of the clocks during the run shows as a difference of the halves
        for name, fn in legs[:2] + legs:
            res.setdefault(name, []).append(timed(fn))
        e.synchronize()
        res["valid_fraction"] = float((mask == 255).float().mean())
    med = {k: float(np.median([r["median_ms"] for r in res[k]])) for k, _ in legs}
    res["gray_median_ms"], res["bgr_median_ms"] = med["gray"], med["bgr"]
    res["ratio"] = med["bgr"] / med["gray"]
    res["criterion_ratio_below_3"] = bool(res["ratio"] < 3.0)
    print(json.dumps(res))
    if args.record:
        with open(args.record, "w") as f:
            f.write("pm_rectify_bgr8 against the three pm_rectify_u8 launches it replaces (tools/bench_rectify_bgr.py)\n")
            f.write("=" * 100 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            f.write("MI355X, one %dx%d image, radial-tangential view, HIP events on the handle's stream, same run and handle,\n"
                    "%d calls after %d warm-up calls per leg, ms (gray and bgr were timed twice, interleaved):\n\n" %
                    (cols, rows, args.steps, args.warmup))
            for key, _ in legs:
                for r in res[key]:
                    f.write("  %-10s median %.4f  min %.4f  max %.4f\n" % (key, r["median_ms"], r["min_ms"], r["max_ms"]))
            f.write("\ngray median %.4f ms, bgr median %.4f ms, ratio %.3f (criterion: below 3) -> %s\n" %
                    (med["gray"], med["bgr"], res["ratio"], "met" if res["criterion_ratio_below_3"] else "MISSED"))
            f.write("gray: pm_rectify_u8 of one gray image; bgr: pm_rectify_bgr8, 8-bit output alone; bgr_float: the float image\n"
                    "alone; bgr_all: 8-bit + float + mask.  Event times include the launch gap.  Valid fraction of the view: %.3f\n" %
                    res["valid_fraction"])
    return 0 if res["criterion_ratio_below_3"] else 1


if __name__ == "__main__":
    sys.exit(main())
