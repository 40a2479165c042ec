#!/usr/bin/env python3
"""Times the range-guided illuminant on the device against the host round trip it replaces (a record, not a gate).

  (a) pm_estimate_illuminant_range_guided at rows x cols with EnhanceUnderwater's parameters
      (r = NextEvenInt(cols / 3), eps = 0.01, s = 8; enhance.cpp:60-62): five launches.
  (b) what a caller had to do before it existed: pm_download of D (12 B/px) and of the range map (4 B/px) and
      pm_upload of an illuminant image (12 B/px), pageable host memory; the CPU filter itself is NOT included.

HIP events on the handle's stream around every call; median (and min / max) over --steps calls after --warmup.
Prints one JSON line.  --only a | b restricts the run (e.g. for a kernel trace of (a) alone)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=720)
    ap.add_argument("--cols", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=("a", "b"), default=None)
    args = ap.parse_args()
    import ctypes as C
    import torch
    import pm_ctypes as pm
    rows, cols = args.rows, args.cols
    third = cols // 3
    r, eps, s = third + third % 2, 0.01, 8
    g = torch.Generator(device="cuda").manual_seed(1)
    rng = 40.0 / (torch.rand((rows, cols), device="cuda", generator=g) * 94 + 2)
    rng[torch.rand((rows, cols), device="cuda", generator=g) < 0.2] = 0
    D = torch.rand((rows, cols, 3), device="cuda", generator=g)
    il = torch.empty_like(D)
    h_D, h_rng = np.empty((rows, cols, 3), np.float32), np.empty((rows, cols), np.float32)
    h_il = np.ones((rows, cols, 3), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out = {"rows": rows, "cols": cols, "r": r, "eps": eps, "s": s, "steps": args.steps}
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        stream = torch.cuda.ExternalStream(e.stream())

        def timed(fn):
            for _ in range(args.warmup):
                fn()
            e.synchronize()
            ms = []
            for _ in range(args.steps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                fn()
                t1.record(stream)
                t1.synchronize()
                ms.append(t0.elapsed_time(t1))
            return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}

        def device_filter():
            e.estimate_illuminant_range_guided(D.data_ptr(), rng.data_ptr(), rows, cols, r, eps, s, il.data_ptr())

        def round_trip():
            e._check(e.lib.pm_download(e.h, vp(h_D), D.data_ptr(), h_D.nbytes), "pm_download")
            e._check(e.lib.pm_download(e.h, vp(h_rng), rng.data_ptr(), h_rng.nbytes), "pm_download")
            e._check(e.lib.pm_upload(e.h, il.data_ptr(), vp(h_il), h_il.nbytes), "pm_upload")

        if args.only in (None, "a"):
            out["a_estimate_illuminant_range_guided"] = timed(device_filter)
            out["a_full_resolution_bytes"] = rows * cols * 16
        if args.only in (None, "b"):
            out["b_download_D_range_upload_illuminant"] = timed(round_trip)
            out["b_bytes"] = h_D.nbytes + h_rng.nbytes + h_il.nbytes
    print(json.dumps(out))


if __name__ == "__main__":
    main()
