#!/usr/bin/env python3
"""Times pm_tsdf_mesh (a record, not a gate: the exit status is 0 either way).

The scene and the method of tools/tsdf_timing.py: a volume of 256^3 voxels of 1 cm (128 MiB), trunc 4 cm, cleared and integrated
from the ground-truth disparities of the benchmark's synthetic 1280x720 pair, once from the identity pose and once from a pose
yawed by 3 degrees about the volume's centre.  HIP events on the handle's stream around every call, device counts only (nothing
synchronises inside the timed window), median (min / max) over --steps calls after --warmup, each leg TWICE, interleaved.

Three legs: the count alone (capacities 0), positions + triangles, positions + triangles + normals.  Reported: vertices and
triangles; the bytes a call must read and write -- the volume once (8 B per node), the scratch (the flag byte written and read
twice, the info word written, 16 B per span written, scanned and read) and the streams it fills (the info word and the flag byte
read once more each, 12 B per vertex and stream, 12 B per triangle); the achieved rate beside pm_tsdf_clear's streaming rate from
the same run, the only yardstick this stage has.  What the neighbours of a node cost beyond that comes out of the caches and is
not in the figure.

Prints one JSON line; --record FILE writes the table there, stamped with --sha; --resources FILE: the compiler's resource usage
of the kernels, appended as it is."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from bench_rectify import event_timer
from fuzz_reproject import IDENTITY, rotation

N = 256
VOXEL, TRUNC = 0.01, 0.04


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--record", default=None)
    ap.add_argument("--resources", default=None)
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
    nodes, spans = N ** 3, (N // 64) * N * N
    res = {"steps": args.steps, "warmup": args.warmup, "volume": [N, N, N], "map": [cols, rows]}
    vol = torch.empty(2 * nodes, dtype=torch.float32, device="cuda")
    disp = torch.from_numpy(gt).cuda()
    d_cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        timed = event_timer(e, args.steps, args.warmup)
        e.tsdf_clear(grid, vol.data_ptr())
        e.tsdf_integrate(cam, grid, IDENTITY, disp.data_ptr(), rows, cols, vol.data_ptr())
        res["integrate_counts"] = list(e.tsdf_integrate(cam, grid, pose, disp.data_ptr(), rows, cols, vol.data_ptr(), want_counts=True))
        nv, nt = e.tsdf_mesh(grid, vol.data_ptr())
        res["vertices"], res["triangles"] = nv, nt
        xyz = torch.empty((max(nv, 1), 3), dtype=torch.float32, device="cuda")
        nrm = torch.empty((max(nv, 1), 3), dtype=torch.float32, device="cuda")
        tri = torch.empty((max(nt, 1), 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        legs = {
            "count": lambda: e.tsdf_mesh(grid, vol.data_ptr(), 0, 0, d_counts=d_cnt.data_ptr(), want_counts=False),
            "xyz_tris": lambda: e.tsdf_mesh(grid, vol.data_ptr(), nv, nt, 0.0, xyz.data_ptr(), None, tri.data_ptr(), d_cnt.data_ptr(), False),
            "xyz_tris_normals": lambda: e.tsdf_mesh(grid, vol.data_ptr(), nv, nt, 0.0, xyz.data_ptr(), nrm.data_ptr(), tri.data_ptr(),
                                                    d_cnt.data_ptr(), False),
            "clear": lambda: e.tsdf_clear(grid, vol.data_ptr()),
        }
        order = ["count", "xyz_tris", "xyz_tris_normals"]
        res["legs"] = {}
        for name in order + order:  # every leg twice, interleaved
            res["legs"].setdefault(name, []).append(timed(legs[name]))
        e.synchronize()
        assert tuple(d_cnt.cpu().numpy()) == (nv, nt)
        res["legs"]["clear"] = [timed(legs["clear"])]  # last: it empties the model
        e.synchronize()
    med = {k: float(np.median([r["median_ms"] for r in v])) for k, v in res["legs"].items()}
    res["median_ms"] = med
    count_bytes = (8 + 1 + 1 + 4) * nodes + 3 * 16 * spans
    res["bytes"] = {"count": count_bytes,
                    "xyz_tris": count_bytes + (4 + 1) * nodes + 16 * spans + 12 * nv + 12 * nt,
                    "xyz_tris_normals": count_bytes + (4 + 1) * nodes + 16 * spans + 24 * nv + 12 * nt}
    res["TBs"] = {k: b / (med[k] * 1e-3) / 1e12 for k, b in res["bytes"].items()}
    res["clear_TBs"] = 8 * nodes / (med["clear"] * 1e-3) / 1e12
    print(json.dumps(res))
    if args.record:
        with open(args.record, "w") as f:
            f.write("pm_tsdf_mesh (tools/tsdf_mesh_timing.py)\n" + "=" * 100 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            f.write("MI355X, one handle, HIP events on the handle's stream, same run, %d calls after %d warm-up calls per leg, every leg\n"
                    "timed twice, interleaved; device counts only.  Volume %d^3 voxels of %g m, trunc %g m, integrated from the %dx%d ground\n"
                    "truth of the benchmark's synthetic pair at the identity pose and at one yawed by 3 degrees (%d voxels updated).\n"
                    "The mesh: %d vertices, %d triangles.\n\n"
                    % (args.steps, args.warmup, N, VOXEL, TRUNC, cols, rows, res["integrate_counts"][1], nv, nt))
            for k, rs in res["legs"].items():
                for r in rs:
                    f.write("  %-20s median %.4f ms  min %.4f  max %.4f\n" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
            f.write("\n  bytes a call must move (the volume once, the scratch, the streams; neighbours come out of the caches):\n")
            for k in order:
                f.write("    %-18s %7.1f MB per call, %.3f TB/s\n" % (k, res["bytes"][k] / 1e6, res["TBs"][k]))
            f.write("    %-18s %7.1f MB per call, %.3f TB/s: pm_tsdf_clear, the streaming rate of this run\n"
                    % ("clear", 8 * nodes / 1e6, res["clear_TBs"]))
            f.write("\nEvent times include the launch gaps between the five to seven launches of a call and the copy of the counts.\n")
            if args.resources:
                f.write("\n" + open(args.resources).read())
    return 0


if __name__ == "__main__":
    sys.exit(main())
