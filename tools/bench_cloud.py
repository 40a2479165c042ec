#!/usr/bin/env python3
"""Times the point-cloud stages (pm_backproject, pm_planes_normals, pm_point_cloud) beside pm_disp_to_range.

One run, one plane-mode handle.  The map is a REAL match's: a PM_MODE_PLANES pm_match_device of a synthetic 1280x720 pair
(its cross-check and background mask leave the zeros a cloud has to skip); at 4096x2160 the same map is tiled to the
size, so that the share of counted pixels is the same at both sizes, and the plane state pm_planes_normals reads is that
of pm_planes_begin at that size (the kernel's work does not depend on what the planes hold).  Legs, each timed with HIP
events on the handle's stream around every call, median (min / max) over --steps calls after --warmup:

  disp_to_range   pm_disp_to_range of the map                       4 B in, 4 B out per pixel
  backproject     pm_backproject of the map                         4 B in, 12 B out per pixel
  planes_normals  pm_planes_normals masked by the map               3 state values + 4 B in, 12 B out per pixel
  cloud_xyz       pm_point_cloud, points + index                    2 x 4 B in per pixel, 16 B out per point
  cloud_all       ... with normals and colour                       ... + 15 B in and 15 B out per point
  cloud_count     capacity 0: the count and offsets launches alone

cloud legs pass d_count and no host count: nothing synchronises inside the timed window.  disp_to_range and backproject
are timed twice, interleaved, so that a drift of the clocks shows as a difference of the halves.  Event times include the
launch gaps: at 1280x720 a single launch is mostly gap.

The criterion (4096x2160): backproject below 3 x disp_to_range -- it moves (4 + 12) / (4 + 4) = 2 x the bytes of a
bandwidth-bound pass; the margin covers 12-byte records that cannot all leave as 16-byte stores.  The three compaction
launches have no parent to compare with: recorded, not judged.  Prints one JSON line; --record FILE writes the table, the
tree's sha (--sha) and the achieved GB/s there.  Exit status 1 when the criterion is missed.

--only LEG --size RxC: that leg alone, 20 calls, no events (for a counter pass of its own under a profiler)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from bench_rectify import event_timer

SIZES = ((720, 1280), (2160, 4096))
CAMERA_720 = (1100.0, 1090.0, 640.3, 359.6, 0.12)  # scaled with the image for the larger size


def camera_for(rows):
    s = rows / 720.0
    return (CAMERA_720[0] * s, CAMERA_720[1] * s, CAMERA_720[2] * s, CAMERA_720[3] * s, CAMERA_720[4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--f16", type=int, default=0)
    ap.add_argument("--record", default=None)
    ap.add_argument("--sha", default="unknown")
    ap.add_argument("--only", default=None)
    ap.add_argument("--size", default=None)
    args = ap.parse_args()
    import torch
    import pm_ctypes as pm
    import synth
    sizes = SIZES if not args.size else (tuple(int(v) for v in args.size.split("x")),)
    big_rows, big_cols = max(r for r, _ in SIZES), max(c for _, c in SIZES)
    res = {"steps": args.steps, "warmup": args.warmup, "state": "f16" if args.f16 else "f32", "sizes": {}}
    prm = pm.default_params(0, patch=7, patchmatch_iters=3, mode=pm.PM_MODE_PLANES, state_dtype=args.f16, max_disp=128)
    with pm.Engine(prm, max_rows=big_rows, max_cols=big_cols) as e:
        # the real match, at 1280x720
        p = synth.make_pair(5, 720, 1280)
        L, R = torch.from_numpy(p["left"]).cuda(), torch.from_numpy(p["right"]).cuda()
        DL = torch.zeros((720, 1280), dtype=torch.float32, device="cuda")
        DR = torch.zeros_like(DL)
        torch.cuda.synchronize()
        e.match_device(1, L.data_ptr(), R.data_ptr(), 720, 1280, None, None, DL.data_ptr(), DR.data_ptr())
        e.synchronize()
        match_map = DL.cpu().numpy()
        res["match_valid_fraction"] = float((match_map > 0).mean())
        timed = event_timer(e, args.steps, args.warmup)
        g = torch.Generator(device="cuda").manual_seed(1)
        for rows, cols in sizes:
            px = rows * cols
            cam = camera_for(rows)
            disp_np = np.tile(match_map, (-(-rows // 720), -(-cols // 1280)))[:rows, :cols]
            disp = torch.from_numpy(np.ascontiguousarray(disp_np)).cuda()
            count = int((disp_np > 0).sum())
            if (rows, cols) != (720, 1280):  # the state of this size: prep + initialisation of a random pair
                img = torch.randint(0, 256, (2, rows, cols), device="cuda", generator=g, dtype=torch.uint8)
                torch.cuda.synchronize()
                e.planes_begin(1, img[0].data_ptr(), img[1].data_ptr(), rows, cols)
            rng_out = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
            xyz = torch.empty((rows, cols, 3), dtype=torch.float32, device="cuda")
            nrm = torch.empty((rows, cols, 3), dtype=torch.float32, device="cuda")
            bgr = torch.randint(0, 256, (rows, cols, 3), device="cuda", generator=g, dtype=torch.uint8)
            c_xyz = torch.empty((count, 3), dtype=torch.float32, device="cuda")
            c_nrm = torch.empty((count, 3), dtype=torch.float32, device="cuda")
            c_bgr = torch.empty((count, 3), dtype=torch.uint8, device="cuda")
            c_idx = torch.empty((count,), dtype=torch.int32, device="cuda")
            d_cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            state_bytes = 3 * (2 if args.f16 else 4)

            def cloud(capacity, full):
                e.point_cloud(cam, disp.data_ptr(), rows, cols, capacity, d_normals=nrm.data_ptr() if full else None,
                              d_bgr8=bgr.data_ptr() if full else None, d_xyz_out=c_xyz.data_ptr(),
                              d_normals_out=c_nrm.data_ptr() if full else None, d_bgr8_out=c_bgr.data_ptr() if full else None,
                              d_index_out=c_idx.data_ptr(), d_count=d_cnt.data_ptr(), host_count=False)

            # leg -> (call, bytes the algorithm moves)
            legs = {
                "disp_to_range": (lambda: e.disp_to_range(disp.data_ptr(), rows, cols, cam[0], cam[4], rng_out.data_ptr()), 8 * px),
                "backproject": (lambda: e.backproject(cam, disp.data_ptr(), rows, cols, xyz.data_ptr()), 16 * px),
                "planes_normals": (lambda: e.planes_normals(0, cam, disp.data_ptr(), rows, cols, nrm.data_ptr()),
                                   (state_bytes + 4 + 12) * px),
                "cloud_xyz": (lambda: cloud(count, False), 8 * px + 16 * count),
                "cloud_all": (lambda: cloud(count, True), 8 * px + (16 + 30) * count),
                "cloud_count": (lambda: cloud(0, False), 4 * px),
            }
            if args.only:
                for _ in range(20):
                    legs[args.only][0]()
                e.synchronize()
                print(json.dumps({"only": args.only, "rows": rows, "cols": cols, "calls": 20}))
                return 0
            e.point_cloud(cam, disp.data_ptr(), rows, cols, 0)  # the block-offset scratch of this size, outside the timing
            order = ["disp_to_range", "backproject"] + list(legs)
            out = {"points": count, "pixels": px, "legs": {}}
            for name in order:
                out["legs"].setdefault(name, []).append(timed(legs[name][0]))
            e.synchronize()
            assert int(d_cnt.cpu()[0]) == count, "pm_point_cloud counted %d, the map has %d" % (int(d_cnt.cpu()[0]), count)
            out["median_ms"] = {k: float(np.median([r["median_ms"] for r in v])) for k, v in out["legs"].items()}
            out["gb_per_s"] = {k: legs[k][1] / (out["median_ms"][k] * 1e-3) / 1e9 for k in legs}
            res["sizes"]["%dx%d" % (cols, rows)] = out
    big = res["sizes"].get("%dx%d" % (big_cols, big_rows))
    if big:
        res["ratio_backproject_over_disp_to_range"] = big["median_ms"]["backproject"] / big["median_ms"]["disp_to_range"]
        res["criterion_ratio_below_3"] = bool(res["ratio_backproject_over_disp_to_range"] < 3.0)
    print(json.dumps(res))
    if args.record:
        with open(args.record, "w") as f:
            f.write("Points, plane-mode normals and the compacted cloud beside pm_disp_to_range (tools/bench_cloud.py)\n")
            f.write("=" * 100 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            f.write("MI355X, one PM_MODE_PLANES handle (%s state), HIP events on the handle's stream, same run,\n"
                    "%d calls after %d warm-up calls per leg (disp_to_range and backproject timed twice, interleaved).\n"
                    "The map: a real plane-mode match of a synthetic 1280x720 pair, %.1f %% of its pixels > 0; tiled to the\n"
                    "larger size.  GB/s = the bytes the stage has to move (see the tool's docstring) over the median.\n\n"
                    % (res["state"], args.steps, args.warmup, 100 * res["match_valid_fraction"]))
            for size, out in res["sizes"].items():
                f.write("%s, %d points of %d pixels, ms:\n" % (size, out["points"], out["pixels"]))
                for k, rs in out["legs"].items():
                    for r in rs:
                        f.write("  %-15s median %.4f  min %.4f  max %.4f\n" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
                f.write("  achieved GB/s: %s\n\n" % ", ".join("%s %.0f" % (k, v) for k, v in out["gb_per_s"].items()))
            if big:
                f.write("%dx%d: backproject median %.4f ms, disp_to_range median %.4f ms, ratio %.3f (criterion: below 3) -> %s\n"
                        % (big_cols, big_rows, big["median_ms"]["backproject"], big["median_ms"]["disp_to_range"],
                           res["ratio_backproject_over_disp_to_range"],
                           "met" if res["criterion_ratio_below_3"] else "MISSED by %.3f" % (res["ratio_backproject_over_disp_to_range"] - 3.0)))
            f.write("Event times include the launch gaps; at 1280x720 a single launch is mostly gap.  The cloud legs are three\n"
                    "launches (count, offsets, scatter; cloud_count: the first two) and are recorded, not judged.\n")
    return 0 if (not big or res["criterion_ratio_below_3"]) else 1


if __name__ == "__main__":
    sys.exit(main())
