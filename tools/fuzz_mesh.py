"""Differential fuzz of pm_grid_mesh (through the C ABI) against the CPU definition (tests/mesh_ref.py).  Random shapes
<= 96x160 (wider than one 256-item segment now and then), disparity maps of quarter-pixel plateaus with every special value
(0, -0.0, negatives, NaN, +inf, subnormals), masks from empty to full, cameras, filters (min_disp, max_range, stride),
max_diff from 0 up, both vertex modes, capacities around both counts and every subset of the optional streams.  Tolerance 0:
bit-exact, guard bands behind both capacities intact, or it prints the case and exits 1.  check_mesh is what
tests/test_mesh.py runs its fixed cases through.

    python tools/fuzz_mesh.py [--cases 60] [--seed 1] [--max-rows 96] [--max-cols 160]
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import mesh_ref as MR
from fuzz_cloud import SPECIALS, Guarded, bits

WIDTH = {"xyz": 12, "normals": 12, "bgr": 3, "index": 4, "tris": 12}
DTYPE = {"xyz": np.float32, "normals": np.float32, "bgr": np.uint8, "index": np.int32, "tris": np.int32}


def plateau_disp(rng, rows, cols, valid=0.7, special=0.05, lo=8.0, spread=3.0):
    """A map of quarter-pixel values within `spread` of a slow ramp, `valid` of its pixels kept, `special` of them drawn
    from SPECIALS, the rest 0: neighbours differ by 0, 0.25, 0.5 ... so that a max_diff of a pixel or so splits the cells
    into joined and cut ones, and equal neighbours exist for max_diff = 0."""
    ramp = lo + 0.05 * np.arange(cols)[None, :] + 0.03 * np.arange(rows)[:, None]
    d = (np.round((ramp + rng.uniform(0, spread, (rows, cols)) * (rng.random((rows, cols)) < 0.5)) * 4) / 4).astype(np.float32)
    d[rng.random((rows, cols)) >= valid] = 0.0
    pick = rng.random((rows, cols)) < special
    d[pick] = rng.choice(SPECIALS, int(pick.sum()))
    return d


def _capacity(spec, count):
    return count if spec == "count" else count - 1 if spec == "count-1" else int(spec)


def check_mesh(torch, e, disp, camera, min_disp=0.0, max_range=0.0, stride=1, max_diff=1.0, vertices=MR.VERTICES_ALL,
               vertex_capacity="count", tri_capacity="count", normal_map=None, bgr=None,
               outputs=("xyz", "normals", "bgr", "index", "tris"), d_counts=True, host_counts=True, want=None):
    """One pm_grid_mesh call against the definition.  The capacities: an int, or "count" / "count-1" (of the definition's
    counts).  outputs: the optional streams that are asked for.  want: the definition's untruncated result for these
    arguments, where the caller has it already.  Returns it."""
    rows, cols = disp.shape
    if want is None:
        want = MR.grid_mesh(disp, camera, min_disp, max_range, stride, max_diff, vertices, None, None, normal_map, bgr)
    nv, nt = want["vertex_count"], want["tri_count"]
    vcap, tcap = _capacity(vertex_capacity, nv), _capacity(tri_capacity, nt)
    if vcap < 0 or tcap < 0:
        return want
    d = torch.from_numpy(disp).cuda()
    dn = torch.from_numpy(np.ascontiguousarray(normal_map, np.float32)).cuda() if normal_map is not None else None
    dc = torch.from_numpy(np.ascontiguousarray(bgr, np.uint8)).cuda() if bgr is not None else None
    bufs = {k: Guarded(torch, WIDTH[k] * (tcap if k == "tris" else vcap)) for k in outputs}
    cnt = Guarded(torch, 8) if d_counts else None
    ptr = lambda k: bufs[k].ptr if k in bufs else None
    n = e.grid_mesh(camera, d.data_ptr(), rows, cols, vcap, tcap, max_diff, vertices, min_disp, max_range, stride,
                    dn.data_ptr() if dn is not None else None, dc.data_ptr() if dc is not None else None, ptr("xyz"),
                    ptr("normals"), ptr("bgr"), ptr("index"), ptr("tris"), cnt.ptr if cnt else None, host_counts)
    e.synchronize()
    if host_counts:
        assert n == (nv, nt), "host counts %s, definition %s" % (n, (nv, nt))
    if cnt:
        got = tuple(int(v) for v in cnt.read(np.int32))
        assert got == (nv, nt), "d_counts %s, definition %s" % (got, (nv, nt))
    for k, buf in bufs.items():
        m = min(nt, tcap) if k == "tris" else min(nv, vcap)
        got = buf.read(DTYPE[k], WIDTH[k] * m)  # records at and beyond min(count, capacity) keep the guard pattern
        assert np.array_equal(bits(got), bits(want[k][:m].ravel())), "pm_grid_mesh: %s differs" % k
    return want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=60)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-rows", type=int, default=96)
    ap.add_argument("--max-cols", type=int, default=160)
    a = ap.parse_args()
    import torch
    import pm_ctypes as pm
    rng = np.random.default_rng(a.seed)
    t0, nv, nt = time.time(), 0, 0
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        for case in range(a.cases):
            rows, cols = int(rng.integers(1, a.max_rows + 1)), int(rng.integers(1, a.max_cols + 1))
            if rng.random() < 0.15:  # more than one segment of a grid row
                rows, cols = int(rng.integers(1, 9)), int(rng.integers(250, 700))
            f = float(rng.uniform(0.4, 2.0) * cols)
            camera = (f * float(rng.choice([1.0, -1.0], p=[0.9, 0.1])), f * float(rng.uniform(0.8, 1.25)),
                      cols / 2 + float(rng.normal(0, 3)), rows / 2 + float(rng.normal(0, 3)), float(rng.uniform(0.02, 0.5)))
            disp = plateau_disp(rng, rows, cols, valid=float(rng.choice([0.0, 0.3, 0.6, 0.9, 1.0])),
                                special=float(rng.choice([0.0, 0.05, 0.3])), spread=float(rng.choice([0.0, 1.0, 3.0])))
            kw = dict(min_disp=float(rng.choice([0.0, 0.0, 9.0, np.inf])),
                      max_range=float(rng.choice([0.0, 0.0, f * 0.1 / 10.0, 1e30])),
                      stride=int(rng.choice([1, 1, 2, 3, 7, 200])),
                      max_diff=float(rng.choice([0.0, 0.25, 0.5, 1.0, 1e30])),
                      vertices=int(rng.choice([MR.VERTICES_ALL, MR.VERTICES_REFERENCED])))
            caps = {}
            for k in ("vertex_capacity", "tri_capacity"):
                c = rng.choice(["count", "count-1", "0", "1", "5", "100000"])
                caps[k] = c if c in ("count", "count-1") else int(c)
            outputs = tuple(k for k in ("xyz", "normals", "bgr", "index", "tris") if rng.random() < 0.7)
            normal_map = rng.normal(size=(rows, cols, 3)).astype(np.float32) if "normals" in outputs or rng.random() < 0.3 else None
            bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8) if "bgr" in outputs or rng.random() < 0.3 else None
            what = dict(case=case, rows=rows, cols=cols, camera=camera, outputs=outputs, **kw, **caps)
            try:
                w = check_mesh(torch, e, disp, camera, normal_map=normal_map, bgr=bgr, outputs=outputs,
                               d_counts=bool(rng.random() < 0.7), host_counts=bool(rng.random() < 0.7), **kw, **caps)
                nv, nt = nv + w["vertex_count"], nt + w["tri_count"]
            except AssertionError as err:
                print("MISMATCH", what, err)
                sys.exit(1)
    print("fuzz_mesh: %d cases (seed %d), %d vertices and %d triangles counted, bit-identical to the definition, %.1f s"
          % (a.cases, a.seed, nv, nt, time.time() - t0))


if __name__ == "__main__":
    main()
