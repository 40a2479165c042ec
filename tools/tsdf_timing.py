#!/usr/bin/env python3
"""Times pm_tsdf_integrate and pm_tsdf_raycast (a record, not a gate: the exit status is 0 either way).

Volume 256^3 voxels of 1 cm (128 MiB), trunc 4 cm, max_weight 64; the map: the ground-truth disparities of the benchmark's
synthetic 1280x720 pair (synth.make_pair(0, 720, 1280)) under a camera whose fx * baseline puts their median 2 m away, the
volume centred on the optical axis from 0.3 m on.  The volume is cleared and integrated once from the identity pose; the timed
integrates then run from a pose yawed by 3 degrees about the volume's centre (so that every call does the same work: the
weights are far from max_weight after warm-up + steps calls), the timed raycasts from that pose too (min_range 0.3, max_range
3, step 0.5: ds = 2 cm).  HIP events on the handle's stream around every call, device counts only (nothing synchronises inside
the timed window), median (min / max) over --steps calls after --warmup, each leg TWICE, interleaved.

Reported: the integrate's achieved bytes per second -- 16 bytes per updated voxel (its record read and written) plus the 4-byte
map once -- beside the 6.29 TB/s a float4 copy reaches on this part; the raycast's time per sample, samples = pixels x the
samples of a ray (every ray takes all of them unless it hits or meets a back face: the figure is an upper bound on the samples
and so a lower bound on the time per sample actually taken).

Prints one JSON line; --record FILE writes the table there, stamped with --sha."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from bench_rectify import event_timer
from fuzz_reproject import IDENTITY, rotation

COPY_TBS = 6.29  # a float4 copy on the MI355X (HBM3E, 8.0 TB/s spec)
N = 256
VOXEL, TRUNC = 0.01, 0.04
RAY = dict(min_range=0.3, max_range=3.0, step=0.5, min_weight=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--record", default=None)
    ap.add_argument("--sha", default="unknown")
    args = ap.parse_args()
    assert args.steps >= 20
    import torch
    import pm_ctypes as pm
    import synth
    import tsdf_ref as TR
    rows, cols = 720, 1280
    gt = synth.make_pair(0, rows, cols)["gt"].astype(np.float32)
    fx = 1000.0
    cam = (fx, fx, cols / 2 - 0.3, rows / 2 + 0.4, 2.0 * float(np.median(gt)) / fx)
    ext = (N - 1) * VOXEL
    grid = TR.make_grid(N, N, N, (-ext / 2, -ext / 2, 0.3), VOXEL, TRUNC, 64.0)
    centre = np.array([0.0, 0.0, 0.3 + ext / 2])
    Rwc = rotation((0, 1, 0), 3.0)
    c = centre + Rwc @ np.array([0.0, 0.0, -centre[2]])
    pose = (Rwc.T.ravel(), -(Rwc.T @ c))
    samples = TR.sample_count(RAY["min_range"], RAY["max_range"], RAY["step"], TRUNC)
    res = {"steps": args.steps, "warmup": args.warmup, "volume": [N, N, N], "map": [cols, rows], "samples_per_ray": samples}
    vol = torch.empty(2 * N ** 3, dtype=torch.float32, device="cuda")
    disp = torch.from_numpy(gt).cuda()
    out = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    nrm = torch.empty((rows, cols, 3), dtype=torch.float32, device="cuda")
    d_cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        timed = event_timer(e, args.steps, args.warmup)
        e.tsdf_clear(grid, vol.data_ptr())
        res["first_integrate"] = list(e.tsdf_integrate(cam, grid, IDENTITY, disp.data_ptr(), rows, cols, vol.data_ptr(), want_counts=True))
        res["integrate_counts"] = list(e.tsdf_integrate(cam, grid, pose, disp.data_ptr(), rows, cols, vol.data_ptr(), want_counts=True))
        res["hits"] = e.tsdf_raycast(cam, grid, pose, vol.data_ptr(), rows, cols, d_disp_out=out.data_ptr(),
                                     d_normals_out=nrm.data_ptr(), want_counts=True, **RAY)
        legs = {
            "clear": lambda: e.tsdf_clear(grid, vol.data_ptr()),
            "integrate": lambda: e.tsdf_integrate(cam, grid, pose, disp.data_ptr(), rows, cols, vol.data_ptr(), d_counts=d_cnt.data_ptr()),
            "raycast_map": lambda: e.tsdf_raycast(cam, grid, pose, vol.data_ptr(), rows, cols, d_disp_out=out.data_ptr(),
                                                  d_counts=d_cnt.data_ptr(), **RAY),
            "raycast_map_normals": lambda: e.tsdf_raycast(cam, grid, pose, vol.data_ptr(), rows, cols, d_disp_out=out.data_ptr(),
                                                          d_normals_out=nrm.data_ptr(), d_counts=d_cnt.data_ptr(), **RAY),
        }
        order = ["integrate", "raycast_map", "raycast_map_normals"]
        res["legs"] = {}
        for name in order + order:  # every leg twice, interleaved
            res["legs"].setdefault(name, []).append(timed(legs[name]))
        res["legs"]["clear"] = [timed(legs["clear"])]  # last: it empties the model
        e.synchronize()
    med = {k: float(np.median([r["median_ms"] for r in v])) for k, v in res["legs"].items()}
    res["median_ms"] = med
    bytes_integrate = 16 * res["integrate_counts"][1] + 4 * rows * cols
    res["integrate_bytes"] = bytes_integrate
    res["integrate_TBs"] = bytes_integrate / (med["integrate"] * 1e-3) / 1e12
    res["integrate_ns_per_voxel"] = med["integrate"] * 1e6 / N ** 3
    res["clear_TBs"] = 8 * N ** 3 / (med["clear"] * 1e-3) / 1e12
    res["raycast_ns_per_sample"] = med["raycast_map"] * 1e6 / (rows * cols * samples)
    print(json.dumps(res))
    if args.record:
        with open(args.record, "w") as f:
            f.write("pm_tsdf_integrate and pm_tsdf_raycast (tools/tsdf_timing.py)\n" + "=" * 100 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            f.write("MI355X, one handle, HIP events on the handle's stream, same run, %d calls after %d warm-up calls per leg, every leg\n"
                    "timed twice, interleaved; device counts only.  Volume %d^3 voxels of %g m, trunc %g m; map %dx%d (the ground truth\n"
                    "of the benchmark's synthetic pair); the timed calls from a pose yawed by 3 degrees about the volume's centre.\n"
                    "Raycast: min_range %g, max_range %g, step %g: %d samples per ray at the most.\n\n"
                    % (args.steps, args.warmup, N, VOXEL, TRUNC, cols, rows, RAY["min_range"], RAY["max_range"], RAY["step"], samples))
            for k, rs in res["legs"].items():
                for r in rs:
                    f.write("  %-20s median %.4f ms  min %.4f  max %.4f\n" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
            f.write("\n  integrate: %d of %d voxels in view, %d updated; 16 B per updated voxel + the map = %.1f MB per call:\n"
                    "             %.3f TB/s against the %.2f TB/s of a float4 copy; %.3f ns per voxel of the grid\n"
                    % (res["integrate_counts"][0], N ** 3, res["integrate_counts"][1], bytes_integrate / 1e6, res["integrate_TBs"],
                       COPY_TBS, res["integrate_ns_per_voxel"]))
            f.write("  clear:     %.1f MB per call, %.3f TB/s\n" % (8 * N ** 3 / 1e6, res["clear_TBs"]))
            f.write("  raycast:   %d of %d pixels hit; %.4f ns per sample (pixels x %d samples: an upper bound on the samples taken)\n"
                    % (res["hits"], rows * cols, res["raycast_ns_per_sample"], samples))
            f.write("\nEvent times include the launch gaps and the 16-byte memset and copy of the counts.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
