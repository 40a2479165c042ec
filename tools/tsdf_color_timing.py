#!/usr/bin/env python3
"""Times the colour volume's stages beside pm_tsdf_integrate (a record, not a gate: the exit status is 0 either way).

The setup is tools/tsdf_timing.py's: a volume of 256^3 voxels of 1 cm, trunc 4 cm; the map is the ground truth of the benchmark's
synthetic 1280x720 pair, its left image (grey, as three equal bytes) the colour; one integrate from the identity pose, the
timed calls from a pose yawed by 3 degrees.  HIP events on the handle's stream around every call, device counts only, median
(min / max) over --steps calls after --warmup, each leg TWICE, interleaved.  Legs: integrate (the plain one), integrate_color
with a byte image at band 0.5 and 1, color_map of the model's render at that pose, color_points of the mesh's vertices,
color_clear.

Reported: the bytes each colour leg moves -- 32 per coloured voxel (its record read and written) beside the integrate's 16 per
updated voxel, plus the map and the image; 16 per corner read by a gather -- and what that is against the 6.29 TB/s of a float4
copy.

Prints one JSON line; --record FILE writes the table there, stamped with --sha."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from bench_rectify import event_timer
from fuzz_reproject import IDENTITY, rotation
from tsdf_timing import COPY_TBS, N, RAY, TRUNC, VOXEL


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
    pair = synth.make_pair(0, rows, cols)
    gt = pair["gt"].astype(np.float32)
    fx = 1000.0
    cam = (fx, fx, cols / 2 - 0.3, rows / 2 + 0.4, 2.0 * float(np.median(gt)) / fx)
    ext = (N - 1) * VOXEL
    grid = TR.make_grid(N, N, N, (-ext / 2, -ext / 2, 0.3), VOXEL, TRUNC, 64.0)
    centre = np.array([0.0, 0.0, 0.3 + ext / 2])
    Rwc = rotation((0, 1, 0), 3.0)
    c = centre + Rwc @ np.array([0.0, 0.0, -centre[2]])
    pose = (Rwc.T.ravel(), -(Rwc.T @ c))
    res = {"steps": args.steps, "warmup": args.warmup, "volume": [N, N, N], "map": [cols, rows]}
    vol = torch.empty(2 * N ** 3, dtype=torch.float32, device="cuda")
    col = torch.empty(4 * N ** 3, dtype=torch.float32, device="cuda")
    disp = torch.from_numpy(gt).cuda()
    image = torch.from_numpy(np.ascontiguousarray(np.repeat(pair["left"][..., None], 3, -1).astype(np.uint8))).cuda()
    render = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    out = torch.empty((rows, cols, 3), dtype=torch.float32, device="cuda")
    out8 = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((4,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        timed = event_timer(e, args.steps, args.warmup)
        e.tsdf_clear(grid, vol.data_ptr())
        e.tsdf_color_clear(grid, col.data_ptr())
        integ = lambda band, p, **kw: e.tsdf_integrate_color(cam, grid, p, disp.data_ptr(), rows, cols, vol.data_ptr(), col.data_ptr(),
                                                             d_bgr8=image.data_ptr(), band=band, **kw)
        res["first_integrate"] = list(integ(1.0, IDENTITY, want_counts=True))
        res["counts_band_1"] = list(integ(1.0, pose, want_counts=True))
        res["counts_band_0.5"] = list(integ(0.5, pose, want_counts=True))
        res["hits"] = e.tsdf_raycast(cam, grid, pose, vol.data_ptr(), rows, cols, d_disp_out=render.data_ptr(), want_counts=True, **RAY)
        res["map_colored"] = e.tsdf_color_map(cam, grid, pose, col.data_ptr(), render.data_ptr(), rows, cols, d_bgr_out=out.data_ptr(),
                                              want_counts=True)
        vertices, _ = e.tsdf_mesh(grid, vol.data_ptr())
        xyz = torch.empty((max(vertices, 1), 3), dtype=torch.float32, device="cuda")
        pts8 = torch.empty((max(vertices, 1), 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        e.tsdf_mesh(grid, vol.data_ptr(), vertices, 0, d_xyz_out=xyz.data_ptr())
        res["vertices"] = vertices
        res["points_colored"] = e.tsdf_color_points(grid, col.data_ptr(), xyz.data_ptr(), vertices, d_bgr8_out=pts8.data_ptr(),
                                                    want_counts=True)
        legs = {
            "integrate": lambda: e.tsdf_integrate(cam, grid, pose, disp.data_ptr(), rows, cols, vol.data_ptr(), d_counts=d_cnt.data_ptr()),
            "integrate_color_0.5": lambda: integ(0.5, pose, d_counts=d_cnt.data_ptr()),
            "integrate_color_1": lambda: integ(1.0, pose, d_counts=d_cnt.data_ptr()),
            "color_map": lambda: e.tsdf_color_map(cam, grid, pose, col.data_ptr(), render.data_ptr(), rows, cols, byte_scale=1.0,
                                                  d_bgr_out=out.data_ptr(), d_bgr8_out=out8.data_ptr(), d_counts=d_cnt.data_ptr()),
            "color_points": lambda: e.tsdf_color_points(grid, col.data_ptr(), xyz.data_ptr(), vertices, d_bgr8_out=pts8.data_ptr(),
                                                        d_counts=d_cnt.data_ptr()),
            "color_clear": lambda: e.tsdf_color_clear(grid, col.data_ptr()),
        }
        order = ["integrate", "integrate_color_0.5", "integrate_color_1", "color_map", "color_points"]
        res["legs"] = {}
        for name in order + order:  # every leg twice, interleaved
            res["legs"].setdefault(name, []).append(timed(legs[name]))
        res["legs"]["color_clear"] = [timed(legs["color_clear"])]  # last: it empties the colour
        e.synchronize()
    med = {k: float(np.median([r["median_ms"] for r in v])) for k, v in res["legs"].items()}
    res["median_ms"] = med
    px = rows * cols
    tbs = lambda b, ms: b / (ms * 1e-3) / 1e12
    res["bytes"] = {
        "integrate": 16 * res["counts_band_1"][1] + 4 * px,
        "integrate_color_0.5": 16 * res["counts_band_0.5"][1] + 32 * res["counts_band_0.5"][2] + 4 * px + 3 * res["counts_band_0.5"][2],
        "integrate_color_1": 16 * res["counts_band_1"][1] + 32 * res["counts_band_1"][2] + 4 * px + 3 * res["counts_band_1"][2],
        "color_map": 4 * px + 128 * res["hits"] + 15 * px,
        "color_points": 12 * vertices + 128 * vertices + 3 * vertices,
        "color_clear": 16 * N ** 3,
    }
    res["TBs"] = {k: tbs(res["bytes"][k], med[k]) for k in med}
    print(json.dumps(res))
    if args.record:
        with open(args.record, "w") as f:
            f.write("pm_tsdf_integrate_color, pm_tsdf_color_map, pm_tsdf_color_points, pm_tsdf_color_clear (tools/tsdf_color_timing.py)\n" + "=" * 100 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            f.write("MI355X, one handle, HIP events on the handle's stream, same run, %d calls after %d warm-up calls per leg, every leg\n"
                    "timed twice, interleaved; device counts only.  Volume %d^3 voxels of %g m, trunc %g m; map %dx%d (the ground truth\n"
                    "of the benchmark's synthetic pair, its left image as three equal bytes); the timed calls from a pose yawed by 3 degrees.\n\n"
                    % (args.steps, args.warmup, N, VOXEL, TRUNC, cols, rows))
            for k, rs in res["legs"].items():
                for r in rs:
                    f.write("  %-20s median %.4f ms  min %.4f  max %.4f\n" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
            f.write("\n  in view, updated, coloured at band 1:   %s\n  in view, updated, coloured at band 0.5: %s\n"
                    % (res["counts_band_1"], res["counts_band_0.5"]))
            f.write("  render: %d of %d pixels hit, %d coloured; mesh: %d vertices, %d coloured\n\n"
                    % (res["hits"], px, res["map_colored"], vertices, res["points_colored"]))
            f.write("  bytes per call (16 per updated voxel, 32 + the pixel's 3 per coloured voxel, the map once; 128 per gathered pixel or\n"
                    "  point at the most, their inputs and outputs) and what that is against the %.2f TB/s of a float4 copy:\n" % COPY_TBS)
            for k in med:
                f.write("  %-20s %8.1f MB  %.3f TB/s\n" % (k, res["bytes"][k] / 1e6, res["TBs"][k]))
            f.write("\nEvent times include the launch gaps and the 16-byte memset and copy of the counts.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
