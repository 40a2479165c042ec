#!/usr/bin/env python3
"""Times pm_bgr_luma, pm_align_photo_evaluate and pm_align_color_disparity beside pm_align_evaluate and pm_align_disparity (a
record, not a gate: the exit status is 0 either way).

1280x720.  The model is the render of tools/tsdf_timing.py's volume (256^3 voxels of 1 cm, the ground-truth map of the
benchmark's synthetic pair and its left image integrated once, with colour, from the identity pose) at a pose yawed by 3 degrees
about the volume's centre: its map, its normals and its colour, as pm_tsdf_raycast and pm_tsdf_color_map leave them on the
device.  The new frame is the render, with its colour, 0.3 degrees further on.  HIP events on the handle's stream around every
call that only enqueues, device outputs only, median (min / max) over --steps calls after --warmup, each leg TWICE, interleaved:
  luma              one pm_bgr_luma of the model's float image, zero_is_absent = 1
  photo_evaluate    one pm_align_photo_evaluate under the identity, the record alone (d_sums)
  evaluate          one pm_align_evaluate under the identity, the record alone: the geometric term beside it
and on the host's clock, because they synchronise: a whole pm_align_color_disparity and a whole pm_align_disparity from the
identity, with their iteration counts.

Prints one JSON line; --record FILE writes the table there, stamped with --sha."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from align_timing import OPT, host_timed
from bench_rectify import event_timer
from fuzz_reproject import IDENTITY, rotation
from tsdf_timing import N, RAY, TRUNC, VOXEL

COLOR = dict(OPT, huber_levels=20.0, lam=0.03)
PHOTO = dict(min_disp=OPT["min_disp"], max_diff=OPT["max_diff"], huber_levels=COLOR["huber_levels"])


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
    res = {"steps": args.steps, "warmup": args.warmup, "volume": [N, N, N], "map": [cols, rows], "options": COLOR}
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    vol, col, disp = f32(2 * N ** 3), f32(4 * N ** 3), torch.from_numpy(gt).cuda()
    image = torch.from_numpy(np.ascontiguousarray(np.repeat(np.asarray(pair["left"], np.uint8)[..., None], 3, -1))).cuda()
    model, normals, bgr_model = f32(rows, cols), f32(rows, cols, 3), f32(rows, cols, 3)
    new, bgr_new = f32(rows, cols), f32(rows, cols, 3)
    luma_model, luma_new, luma_out = f32(rows, cols), f32(rows, cols), f32(rows, cols)
    d_sums = torch.zeros((30,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        timed = event_timer(e, args.steps, args.warmup)
        e.tsdf_clear(grid, vol.data_ptr())
        e.tsdf_color_clear(grid, col.data_ptr())
        e.tsdf_integrate_color(cam, grid, IDENTITY, disp.data_ptr(), rows, cols, vol.data_ptr(), col.data_ptr(), d_bgr8=image.data_ptr())
        for p, d_out, n_out, c_out, key in ((pose, model, normals, bgr_model, "model"), (pose_new, new, None, bgr_new, "new")):
            res[key + "_hits"] = e.tsdf_raycast(cam, grid, p, vol.data_ptr(), rows, cols, d_disp_out=d_out.data_ptr(),
                                                d_normals_out=n_out.data_ptr() if n_out is not None else None, want_counts=True, **RAY)
            res[key + "_colored"] = e.tsdf_color_map(cam, grid, p, col.data_ptr(), d_out.data_ptr(), rows, cols,
                                                     d_bgr_out=c_out.data_ptr(), want_counts=True)
        e.bgr_luma(rows, cols, luma_model.data_ptr(), d_bgr=bgr_model.data_ptr(), zero_is_absent=True)
        e.bgr_luma(rows, cols, luma_new.data_ptr(), d_bgr=bgr_new.data_ptr(), zero_is_absent=False)
        geo = (model.data_ptr(), normals.data_ptr(), new.data_ptr())
        photo = (model.data_ptr(), luma_model.data_ptr(), new.data_ptr(), luma_new.data_ptr())
        s = e.align_photo_evaluate(cam, *photo, rows, cols, None, PHOTO, want_sums=True)
        res["photo_counts"] = [s.n_model, s.n_gate, s.n_used]
        s = e.align_evaluate(cam, *geo, rows, cols, None, OPT, want_sums=True)
        res["evaluate_counts"] = [s.n_model, s.n_gate, s.n_used]
        color_call = lambda: e.align_color_disparity(cam, model.data_ptr(), normals.data_ptr(), bgr_model.data_ptr(), new.data_ptr(), rows,
                                                     cols, d_bgr_new=bgr_new.data_ptr(), options=COLOR)
        _, _, cinfo = color_call()
        res["align_color"] = dict(cinfo["geo"], n_photo_used=cinfo["n_photo_used"], rms_levels=cinfo["rms_levels"])
        res["align_color"].pop("H")
        _, _, ginfo = e.align_disparity(cam, *geo, rows, cols, None, OPT)
        res["align"] = {k: ginfo[k] for k in ("valid", "n_used", "iterations", "rms_px")}
        legs = {
            "luma": lambda: e.bgr_luma(rows, cols, luma_out.data_ptr(), d_bgr=bgr_model.data_ptr(), zero_is_absent=True),
            "photo_evaluate": lambda: e.align_photo_evaluate(cam, *photo, rows, cols, None, PHOTO, d_sums=d_sums.data_ptr()),
            "evaluate": lambda: e.align_evaluate(cam, *geo, rows, cols, None, OPT, d_sums=d_sums.data_ptr()),
        }
        host_legs = {
            "align_color_disparity_host_clock": color_call,
            "align_disparity_host_clock": lambda: e.align_disparity(cam, *geo, rows, cols, None, OPT),
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
            f.write("pm_bgr_luma, pm_align_photo_evaluate and pm_align_color_disparity beside pm_align_evaluate and pm_align_disparity\n"
                    "(tools/align_color_timing.py)\n" + "=" * 100 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            f.write("MI355X, one handle, same run, %d calls after %d warm-up calls per leg, every leg timed twice, interleaved.  Map %dx%d;\n"
                    "the model is the render (map, normals, colour) of a %d^3-voxel coloured volume of %g m at a pose yawed by 3 degrees, the\n"
                    "new frame the render 0.3 degrees further on.  HIP events on the handle's stream for the legs that only enqueue, the\n"
                    "host's clock for the two calls that synchronise.\n\n" % (args.steps, args.warmup, cols, rows, N, VOXEL))
            for k, rs in res["legs"].items():
                for r in rs:
                    f.write("  %-34s median %.4f ms  min %.4f  max %.4f\n" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
            c, a = res["align_color"], res["align"]
            f.write("\n  photo_evaluate: %d model pixels, %d at the gate, %d used of %d\n" % (*res["photo_counts"], rows * cols))
            f.write("  evaluate:       %d model pixels, %d at the gate, %d used\n" % tuple(res["evaluate_counts"]))
            f.write("  a photometric evaluation costs %.2f x the geometric one beside it\n" % (med["photo_evaluate"] / med["evaluate"]))
            f.write("  align_color_disparity: valid %d, %d iterations (%d pairs of evaluations), %d + %d used, rms %.4f px, %.4f levels:\n"
                    "      %.4f ms per pair with its downloads, blend and solve, against %.4f ms for the four launches alone\n"
                    % (c["valid"], c["iterations"], c["iterations"] + 1, c["n_used"], c["n_photo_used"], c["rms_px"], c["rms_levels"],
                       med["align_color_disparity_host_clock"] / (c["iterations"] + 1), med["photo_evaluate"] + med["evaluate"]))
            f.write("  align_disparity:       valid %d, %d iterations, %d used, rms %.4f px\n" % (a["valid"], a["iterations"], a["n_used"], a["rms_px"]))
            f.write("\nEvent times include the launch gaps and the 16-byte memset of the counts.  Fusing the two evaluations into one kernel\n"
                    "would save at most the smaller of the two event times per update and would change the order of the sum.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
