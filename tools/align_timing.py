#!/usr/bin/env python3
"""Times pm_align_evaluate and pm_align_disparity beside the stages they stand next to (a record, not a gate: the exit status is
0 either way).

1280x720.  The model is the render of tools/tsdf_timing.py's volume (256^3 voxels of 1 cm, the ground-truth map of the
benchmark's synthetic pair integrated once from the identity pose) at a pose yawed by 3 degrees about the volume's centre: its
map and its normals, as pm_tsdf_raycast leaves them on the device.  The new frame is the render 0.3 degrees further on.  HIP
events on the handle's stream around every call, device outputs only (nothing synchronises inside the timed window), median
(min / max) over --steps calls after --warmup, each leg TWICE, interleaved:
  evaluate          one pm_align_evaluate under the identity, the record alone (d_sums)
  evaluate_planes   the same with d_class_out and d_residual_out
  raycast           pm_tsdf_raycast, map and normals, at the same size: the stage in front of it
and on the host's clock, because they synchronise: a whole pm_align_disparity from the identity with its iteration count, and
pm_estimate_motion (cell 16, p = 5, s = 12; the pair's left image against itself) as the other source of a pose.

Prints one JSON line; --record FILE writes the table there, stamped with --sha."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from bench_rectify import event_timer
from fuzz_reproject import IDENTITY, rotation
from tsdf_timing import N, RAY, TRUNC, VOXEL

OPT = dict(min_disp=0.0, max_diff=2.0, huber_px=1.0, iterations=10, epsilon=1e-7, min_used=1000)
TRACK = dict(cell=16, patch_radius=5, search_radius=12, min_score=1, min_disp=0.0, max_disp=0.0, max_sad=0, min_gap=0)


def host_timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


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

    def arc(degrees):
        Rwc = rotation((0, 1, 0), degrees)
        c = centre + Rwc @ np.array([0.0, 0.0, -centre[2]])
        return Rwc.T.ravel(), -(Rwc.T @ c)

    pose, pose_new = arc(3.0), arc(3.3)
    res = {"steps": args.steps, "warmup": args.warmup, "volume": [N, N, N], "map": [cols, rows], "options": OPT}
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    vol, disp = f32(2 * N ** 3), torch.from_numpy(gt).cuda()
    model, normals, new, residual, scratch_n = f32(rows, cols), f32(rows, cols, 3), f32(rows, cols), f32(rows, cols), f32(rows, cols, 3)
    classes = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
    d_sums = torch.zeros((30,), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
    left = torch.from_numpy(np.ascontiguousarray(pair["left"])).cuda()
    torch.cuda.synchronize()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        timed = event_timer(e, args.steps, args.warmup)
        e.tsdf_clear(grid, vol.data_ptr())
        e.tsdf_integrate(cam, grid, IDENTITY, disp.data_ptr(), rows, cols, vol.data_ptr())
        res["model_hits"] = e.tsdf_raycast(cam, grid, pose, vol.data_ptr(), rows, cols, d_disp_out=model.data_ptr(),
                                           d_normals_out=normals.data_ptr(), want_counts=True, **RAY)
        res["new_hits"] = e.tsdf_raycast(cam, grid, pose_new, vol.data_ptr(), rows, cols, d_disp_out=new.data_ptr(), want_counts=True, **RAY)
        ptrs = (model.data_ptr(), normals.data_ptr(), new.data_ptr())
        s = e.align_evaluate(cam, *ptrs, rows, cols, None, OPT, want_sums=True)
        res["evaluate_counts"] = [s.n_model, s.n_gate, s.n_used]
        R, t, info = e.align_disparity(cam, *ptrs, rows, cols, None, OPT)
        res["align"] = {k: info[k] for k in ("valid", "n_model", "n_gate", "n_used", "iterations", "rms_px")}
        _, _, minfo = e.estimate_motion(cam, left.data_ptr(), disp.data_ptr(), left.data_ptr(), rows, cols, None, TRACK, None)
        res["estimate_motion"] = minfo
        legs = {
            "evaluate": lambda: e.align_evaluate(cam, *ptrs, rows, cols, None, OPT, d_sums=d_sums.data_ptr()),
            "evaluate_planes": lambda: e.align_evaluate(cam, *ptrs, rows, cols, None, OPT, classes.data_ptr(), residual.data_ptr(),
                                                        d_sums.data_ptr()),
            "raycast": lambda: e.tsdf_raycast(cam, grid, pose, vol.data_ptr(), rows, cols, d_disp_out=residual.data_ptr(),
                                              d_normals_out=scratch_n.data_ptr(), d_counts=d_cnt.data_ptr(), **RAY),
        }
        host_legs = {
            "align_disparity_host_clock": lambda: e.align_disparity(cam, *ptrs, rows, cols, None, OPT),
            "estimate_motion_host_clock": lambda: e.estimate_motion(cam, left.data_ptr(), disp.data_ptr(), left.data_ptr(), rows, cols,
                                                                    None, TRACK, None),
        }
        res["legs"] = {}
        for _ in range(2):  # every leg twice, interleaved
            for name, fn in legs.items():
                res["legs"].setdefault(name, []).append(timed(fn))
            for name, fn in host_legs.items():
                e.synchronize()
                res["legs"].setdefault(name, []).append(host_timed(fn, args.steps, args.warmup))
        e.synchronize()
    res["median_ms"] = {k: float(np.median([r["median_ms"] for r in v])) for k, v in res["legs"].items()}
    print(json.dumps(res))
    if args.record:
        med = res["median_ms"]
        with open(args.record, "w") as f:
            f.write("pm_align_evaluate and pm_align_disparity beside pm_tsdf_raycast and pm_estimate_motion (tools/align_timing.py)\n" + "=" * 100 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            f.write("MI355X, one handle, same run, %d calls after %d warm-up calls per leg, every leg timed twice, interleaved.  Map %dx%d;\n"
                    "the model is the render (map and normals) of a %d^3-voxel volume of %g m at a pose yawed by 3 degrees, the new frame\n"
                    "the render 0.3 degrees further on.  HIP events on the handle's stream for the legs that only enqueue, the host's clock\n"
                    "for the two calls that synchronise.\n\n" % (args.steps, args.warmup, cols, rows, N, VOXEL))
            for k, rs in res["legs"].items():
                for r in rs:
                    f.write("  %-28s median %.4f ms  min %.4f  max %.4f\n" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
            a = res["align"]
            f.write("\n  evaluate: %d model pixels, %d at the gate, %d used of %d\n" % (*res["evaluate_counts"], rows * cols))
            f.write("  align_disparity: valid %d, %d iterations (%d evaluations), %d used, rms %.4f px: %.4f ms per evaluation with its\n"
                    "                   download and solve, against %.4f ms for the launches alone\n"
                    % (a["valid"], a["iterations"], a["iterations"] + 1, a["n_used"], a["rms_px"],
                       med["align_disparity_host_clock"] / (a["iterations"] + 1), med["evaluate"]))
            f.write("  an evaluation costs %.2f x the raycast in front of it\n" % (med["evaluate"] / med["raycast"]))
            f.write("  estimate_motion: %s\n" % json.dumps(res["estimate_motion"]))
            f.write("\nEvent times include the launch gaps and the 16-byte memset of the counts.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
