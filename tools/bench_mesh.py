#!/usr/bin/env python3
"""Times pm_grid_mesh beside its yardstick, pm_point_cloud (points + index), on the same handle, map and run.

The map is a REAL match's, as in tools/bench_cloud.py: a PM_MODE_PLANES pm_match_device of a synthetic 1280x720 pair (its
cross-check and background mask leave the zeros a mesh has to cut around); at 4096x2160 the same map is tiled to the size.
Stride 1, max_diff 1.  Legs, each timed with HIP events on the handle's stream around every call, median (min / max) over
--steps calls after --warmup, every leg TWICE, interleaved, so that a drift of the clocks shows as a difference of the
halves:

  cloud_xyz        pm_point_cloud, points + index                               three launches
  mesh_all         pm_grid_mesh, PM_MESH_VERTICES_ALL, xyz + index + triangles   five launches
  mesh_referenced  ... PM_MESH_VERTICES_REFERENCED
  mesh_full        ... REFERENCED with normals and colour as well
  mesh_count       both capacities 0: the count and the two offsets launches alone

Every leg passes device counts and no host counts: nothing synchronises inside the timed window.  Event times include the
launch gaps: at 1280x720 five launches of a few microseconds each are mostly gap -- recorded, not judged.

The budget (4096x2160 only, for mesh_all and mesh_referenced):   t_mesh / t_cloud <= 1.5 * (B_mesh / B_cloud)
with B the bytes each stage must move for that map, N grid items, V vertices, T triangles, P points, all measured:
  B_cloud = 2 * 4 N + 16 P                 the map once in the count and once in the scatter launch; 12 + 4 B per point
  B_mesh  = 3 * 4 N + 2 * 4 N + 16 V + 12 T  the map once in each of the three launches that read it; the slot map written
                                           once and read once; 12 + 4 B per vertex; 12 B per triangle
The factor 1.5 allows for 12-byte triangle records and the halo rows.  mesh_full adds 15 B in and 15 B out per vertex and
is recorded, not judged.  Prints one JSON line; --record FILE writes the formula, the counts, the times, the ratios and
met / missed there, stamped with --sha.  Exit status 1 when the budget is missed.

--only LEG --size RxC: that leg alone, 20 calls, no events (for a counter pass of its own under a profiler)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from bench_cloud import SIZES, camera_for
from bench_rectify import event_timer

MAX_DIFF = 1.0
FACTOR = 1.5
JUDGED = ("mesh_all", "mesh_referenced")


def cloud_bytes(n, points):
    return 2 * 4 * n + 16 * points


def mesh_bytes(n, vertices, tris, full=False):
    return 3 * 4 * n + 2 * 4 * n + 16 * vertices + 12 * tris + (30 * vertices if full else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
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
    res = {"steps": args.steps, "warmup": args.warmup, "max_diff": MAX_DIFF, "factor": FACTOR, "sizes": {}}
    prm = pm.default_params(0, patch=7, patchmatch_iters=3, mode=pm.PM_MODE_PLANES, max_disp=128)
    with pm.Engine(prm, max_rows=720, max_cols=1280) as e:
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
            n = rows * cols
            cam = camera_for(rows)
            disp_np = np.tile(match_map, (-(-rows // 720), -(-cols // 1280)))[:rows, :cols]
            disp = torch.from_numpy(np.ascontiguousarray(disp_np)).cuda()
            nrm = torch.empty((rows, cols, 3), dtype=torch.float32, device="cuda").normal_(generator=g)
            bgr = torch.randint(0, 256, (rows, cols, 3), device="cuda", generator=g, dtype=torch.uint8)
            torch.cuda.synchronize()
            # the counts of this map (and the scratch of this size, outside the timing)
            points = e.point_cloud(cam, disp.data_ptr(), rows, cols, 0)
            counts = {mode: e.grid_mesh(cam, disp.data_ptr(), rows, cols, 0, 0, MAX_DIFF, mode)
                      for mode in (pm.PM_MESH_VERTICES_ALL, pm.PM_MESH_VERTICES_REFERENCED)}
            tris = counts[pm.PM_MESH_VERTICES_ALL][1]
            assert counts[pm.PM_MESH_VERTICES_REFERENCED][1] == tris and counts[pm.PM_MESH_VERTICES_ALL][0] == points
            o_xyz = torch.empty((points, 3), dtype=torch.float32, device="cuda")
            o_nrm = torch.empty((points, 3), dtype=torch.float32, device="cuda")
            o_bgr = torch.empty((points, 3), dtype=torch.uint8, device="cuda")
            o_idx = torch.empty((points,), dtype=torch.int32, device="cuda")
            o_tri = torch.empty((max(tris, 1), 3), dtype=torch.int32, device="cuda")
            d_cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def cloud():
                e.point_cloud(cam, disp.data_ptr(), rows, cols, points, d_xyz_out=o_xyz.data_ptr(), d_index_out=o_idx.data_ptr(),
                              d_count=d_cnt.data_ptr(), host_count=False)

            def mesh(mode, full=False, count_only=False):
                e.grid_mesh(cam, disp.data_ptr(), rows, cols, 0 if count_only else points, 0 if count_only else tris, MAX_DIFF, mode,
                            d_normals=nrm.data_ptr() if full else None, d_bgr8=bgr.data_ptr() if full else None,
                            d_xyz_out=o_xyz.data_ptr(), d_normals_out=o_nrm.data_ptr() if full else None,
                            d_bgr8_out=o_bgr.data_ptr() if full else None, d_index_out=o_idx.data_ptr(),
                            d_tri_out=o_tri.data_ptr(), d_counts=d_cnt.data_ptr(), host_counts=False)

            v_all, v_ref = counts[pm.PM_MESH_VERTICES_ALL][0], counts[pm.PM_MESH_VERTICES_REFERENCED][0]
            # leg -> (call, bytes the stage must move)
            legs = {
                "cloud_xyz": (cloud, cloud_bytes(n, points)),
                "mesh_all": (lambda: mesh(pm.PM_MESH_VERTICES_ALL), mesh_bytes(n, v_all, tris)),
                "mesh_referenced": (lambda: mesh(pm.PM_MESH_VERTICES_REFERENCED), mesh_bytes(n, v_ref, tris)),
                "mesh_full": (lambda: mesh(pm.PM_MESH_VERTICES_REFERENCED, full=True), mesh_bytes(n, v_ref, tris, True)),
                "mesh_count": (lambda: mesh(pm.PM_MESH_VERTICES_REFERENCED, count_only=True), 4 * n),
            }
            if args.only:
                for _ in range(20):
                    legs[args.only][0]()
                e.synchronize()
                print(json.dumps({"only": args.only, "rows": rows, "cols": cols, "calls": 20}))
                return 0
            out = {"items": n, "points": points, "vertices_all": v_all, "vertices_referenced": v_ref, "triangles": tris,
                   "bytes": {k: v[1] for k, v in legs.items()}, "legs": {}}
            for name in list(legs) + list(legs):  # every leg twice, interleaved
                out["legs"].setdefault(name, []).append(timed(legs[name][0]))
            e.synchronize()
            assert tuple(int(v) for v in d_cnt.cpu()) == (v_ref, tris), "d_counts of the last leg"
            out["median_ms"] = {k: float(np.median([r["median_ms"] for r in v])) for k, v in out["legs"].items()}
            out["gb_per_s"] = {k: legs[k][1] / (out["median_ms"][k] * 1e-3) / 1e9 for k in legs}
            out["ratio"] = {k: out["median_ms"][k] / out["median_ms"]["cloud_xyz"] for k in JUDGED}
            out["budget"] = {k: FACTOR * legs[k][1] / legs["cloud_xyz"][1] for k in JUDGED}
            res["sizes"]["%dx%d" % (cols, rows)] = out
    big = res["sizes"].get("%dx%d" % (big_cols, big_rows))
    if big:
        res["budget_met"] = {k: bool(big["ratio"][k] <= big["budget"][k]) for k in JUDGED}
    print(json.dumps(res))
    if args.record:
        with open(args.record, "w") as f:
            f.write("pm_grid_mesh beside pm_point_cloud (tools/bench_mesh.py)\n" + "=" * 100 + "\n\n")
            f.write("tree: %s\n" % args.sha)
            f.write("MI355X, one handle, HIP events on the handle's stream, same run, %d calls after %d warm-up calls per leg,\n"
                    "every leg timed twice, interleaved.  The map: a real plane-mode match of a synthetic 1280x720 pair, %.1f %% of\n"
                    "its pixels > 0; tiled to the larger size.  Stride 1, max_diff %.1f.\n\n"
                    "Budget (4096x2160 only):  t_mesh / t_cloud <= %.1f * (B_mesh / B_cloud)\n"
                    "  B_cloud = 2 * 4 N + 16 P                   (N grid items, P points)\n"
                    "  B_mesh  = 3 * 4 N + 2 * 4 N + 16 V + 12 T  (V vertices, T triangles; mesh_full: + 30 V)\n\n"
                    % (args.steps, args.warmup, 100 * res["match_valid_fraction"], MAX_DIFF, FACTOR))
            for size, out in res["sizes"].items():
                f.write("%s: N %d, P %d, V %d (all) / %d (referenced), T %d; ms:\n"
                        % (size, out["items"], out["points"], out["vertices_all"], out["vertices_referenced"], out["triangles"]))
                for k, rs in out["legs"].items():
                    for r in rs:
                        f.write("  %-16s median %.4f  min %.4f  max %.4f\n" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
                f.write("  bytes: %s\n" % ", ".join("%s %d" % (k, v) for k, v in out["bytes"].items()))
                f.write("  achieved GB/s of those bytes: %s\n" % ", ".join("%s %.0f" % (k, v) for k, v in out["gb_per_s"].items()))
                for k in JUDGED:
                    verdict = "recorded, not judged" if out is not big else (
                        "met" if res["budget_met"][k] else "MISSED by %.3f" % (out["ratio"][k] - out["budget"][k]))
                    f.write("  %-16s t_mesh %.4f / t_cloud %.4f = %.3f; budget %.1f * %d / %d = %.3f -> %s\n"
                            % (k, out["median_ms"][k], out["median_ms"]["cloud_xyz"], out["ratio"][k], FACTOR, out["bytes"][k],
                               out["bytes"]["cloud_xyz"], out["budget"][k], verdict))
                f.write("\n")
            f.write("Event times include the launch gaps (five launches for the mesh, three for the cloud); at 1280x720 they are\n"
                    "mostly gap.  Kernel time without the gaps is not measured here.\n")
    return 0 if (not big or all(res["budget_met"].values())) else 1


if __name__ == "__main__":
    sys.exit(main())
