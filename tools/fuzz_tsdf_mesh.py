"""Differential fuzz of pm_tsdf_mesh (through the C ABI) against the CPU definition (tests/tsdf_mesh_ref.py).  Random volumes
<= 140x24x16 whose x extent crosses the 64-node span or not, holding a sphere, a tilted plane or noise, with weights from
{0, 1, 2, 3.5}, exact zeros, NaN and +-inf values, NaN payloads in unobserved records, min_weight 0 / 1 / 2, capacities from 0 to
full, every subset of the outputs and output pointers 4, 8 or 12 bytes past a 16-byte boundary.  Tolerance 0: positions, normals,
triangles and both counts bit-exact, nothing written behind a capacity, guard bands around every buffer intact, the volume
unchanged, or it prints the case and exits 1.  check_tsdf_mesh is what tests/test_tsdf_mesh.py runs its fixed cases through.

    python tools/fuzz_tsdf_mesh.py [--cases 40] [--seed 1]
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import tsdf_mesh_ref as MR
import tsdf_ref as TR
from fuzz_cloud import Guarded, bits  # noqa: F401  (re-exported to the tests)

OUTPUTS = ("xyz", "normals", "tris", "d_counts", "counts")
WEIGHTS = (0.0, 1.0, 2.0, 3.5)


def sphere_volume(shape, radius, centre, trunc, weight=1.0):
    """tsdf = clamp((|node - centre| - radius) / trunc, -1, 1) in voxels, rounded once to binary32; float32 [nz][ny][nx][2]."""
    nx, ny, nz = shape
    k, j, i = np.mgrid[:nz, :ny, :nx].astype(np.float64)
    d = np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2) - radius
    v = np.zeros((nz, ny, nx, 2), np.float32)
    v[..., 0] = np.clip(d / trunc, -1.0, 1.0).astype(np.float32)
    v[..., 1] = weight
    return v


def plane_volume(shape, normal, offset, trunc, weight=1.0):
    nx, ny, nz = shape
    k, j, i = np.mgrid[:nz, :ny, :nx].astype(np.float64)
    n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    v = np.zeros((nz, ny, nx, 2), np.float32)
    v[..., 0] = np.clip((i * n[0] + j * n[1] + k * n[2] - offset) / trunc, -1.0, 1.0).astype(np.float32)
    v[..., 1] = weight
    return v


def random_volume(rng, shape, weights=WEIGHTS):
    nx, ny, nz = shape
    v = np.zeros((nz, ny, nx, 2), np.float32)
    v[..., 0] = rng.uniform(-1, 1, (nz, ny, nx))
    v[..., 1] = rng.choice(weights, (nz, ny, nx))
    return v


def add_specials(rng, v, share=0.02):
    """Into a copy of v: exact zeros (+0.0 and -0.0) and NaN / +-inf values in observed records, NaN payloads, infinities and
    negative or NaN weights in unobserved ones."""
    v = np.ascontiguousarray(v, np.float32).copy()
    f = v.reshape(-1, 2)  # views of v: (tsdf, weight) per node, as values and as words
    u = f.view(np.uint32)
    n = f.shape[0]
    pick = lambda: rng.random(n) < share
    f[pick(), 0] = 0.0
    f[pick(), 0] = -0.0
    for value in (np.nan, np.inf, -np.inf):
        f[rng.random(n) < share / 3, 0] = value
    dead = pick()
    u[dead, 1] = rng.choice(np.array([0x00000000, 0x80000000, 0xBF800000, 0x7FC00001, 0xFF800000], np.uint32), int(dead.sum()))
    u[dead, 0] = rng.choice(np.array([0x7FC00123, 0xFFC00000, 0x7F800000, 0x3F000000, 0x00000001], np.uint32), int(dead.sum()))
    return v


def check_tsdf_mesh(torch, e, grid, voxels, min_weight=0.0, vertex_capacity=None, tri_capacity=None, outputs=OUTPUTS,
                    offset_floats=0, want=None):
    """One call against the definition.  voxels: float32 [nz][ny][nx][2], uploaded into a guarded buffer.  A capacity of None:
    exactly what the definition counts.  outputs: which of the five outputs are asked for.  offset_floats: the outputs start
    that many floats past a 16-byte boundary.  want: the definition's uncut mesh where the caller has it.  Returns it."""
    nodes = grid["nx"] * grid["ny"] * grid["nz"]
    voxels = np.array(voxels, np.float32, order="C")  # a copy: the caller's may be read-only
    full = MR.mesh(grid, voxels, min_weight) if want is None else want
    nv, nt = (int(c) for c in full["counts"])
    vcap = nv if vertex_capacity is None else vertex_capacity
    tcap = nt if tri_capacity is None else tri_capacity
    off = 4 * offset_floats
    volume = Guarded(torch, 8 * nodes)
    volume.t[volume.lo:volume.lo + volume.n] = torch.from_numpy(voxels.view(np.uint8).ravel())
    bufs = {k: Guarded(torch, size, off) for k, size in (("xyz", 12 * vcap), ("normals", 12 * vcap), ("tris", 12 * tcap)) if k in outputs}
    cnt = Guarded(torch, 8) if "d_counts" in outputs else None
    torch.cuda.synchronize()  # the uploads run on torch's stream, the stage on the handle's: nothing else orders them
    n = e.tsdf_mesh(grid, volume.ptr, vcap, tcap, min_weight, *(bufs[k].ptr if k in bufs else None for k in ("xyz", "normals", "tris")),
                    cnt.ptr if cnt else None, "counts" in outputs)
    e.synchronize()
    if "counts" in outputs:
        assert tuple(n) == (nv, nt), "host counts %s, definition %s" % (n, (nv, nt))
    else:
        assert n is None
    if cnt:
        got = cnt.read(np.int32)
        assert tuple(got) == (nv, nt), "d_counts %s, definition %s" % (got, (nv, nt))
    for k, buf in bufs.items():
        records = min(nv, vcap) if k != "tris" else min(nt, tcap)
        w = full[k][:records]
        got = buf.read(np.int32 if k == "tris" else np.float32, 12 * records).reshape(-1, 3)  # and nothing behind them
        bad = np.argwhere(bits(got) != bits(w))
        assert len(bad) == 0, "pm_tsdf_mesh: %d of %d values of %s differ; (record, component, got, want): %s" % (
            len(bad), got.size, k, [(int(r), int(c), got[r, c].item(), w[r, c].item()) for r, c in bad[:6]])
    assert np.array_equal(volume.read(np.uint32), bits(voxels).ravel()), "pm_tsdf_mesh wrote to the volume"
    return full


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import torch
    import pm_ctypes as pm
    rng = np.random.default_rng(a.seed)
    t0, totals = time.time(), np.zeros(2, np.int64)
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        for case in range(a.cases):
            shape = (int(rng.choice([1, 2, 7, 33, 64, 65, 70, 140])), int(rng.integers(1, 25)), int(rng.integers(1, 17)))
            voxel = float(rng.uniform(0.01, 0.05))
            trunc_voxels = float(rng.uniform(1.5, 5.0))
            grid = TR.make_grid(*shape, rng.normal(0, 0.3, 3), voxel, voxel * trunc_voxels)
            kind = str(rng.choice(["sphere", "plane", "noise"]))
            centre = [float(rng.uniform(0.2, 0.8)) * (n - 1) for n in shape]
            if kind == "sphere":
                v = sphere_volume(shape, float(rng.uniform(0.2, 0.6)) * max(min(shape[0], 40), shape[1], shape[2]), centre, trunc_voxels)
            elif kind == "plane":
                v = plane_volume(shape, rng.normal(size=3), float(np.dot(centre, rng.uniform(0.5, 1.5, 3))) / 1.7, trunc_voxels)
            else:
                v = random_volume(rng, shape)
            if rng.random() < 0.6:
                v[..., 1] = rng.choice(WEIGHTS, v.shape[:3], p=(0.1, 0.4, 0.3, 0.2))
            if rng.random() < 0.6:
                v = add_specials(rng, v, float(rng.choice([0.005, 0.05])))
            min_weight = float(rng.choice([0.0, 1.0, 2.0]))
            full = MR.mesh(grid, v, min_weight)
            cap = lambda n: [None, 0, int(rng.integers(0, n + 1)), n + 5][int(rng.integers(0, 4))]
            outputs = tuple(k for k in OUTPUTS if rng.random() < 0.7) or ("counts",)
            what = dict(case=case, shape=shape, kind=kind, min_weight=min_weight, outputs=outputs, counts=tuple(full["counts"]))
            try:
                check_tsdf_mesh(torch, e, grid, v, min_weight, cap(int(full["counts"][0])), cap(int(full["counts"][1])), outputs,
                                int(rng.integers(0, 4)), want=full)
                totals += full["counts"]
            except AssertionError as err:
                print("MISMATCH", what, err)
                sys.exit(1)
    print("fuzz_tsdf_mesh: %d cases (seed %d), %d vertices, %d triangles, bit-identical to the definition, %.1f s"
          % (a.cases, a.seed, *totals, time.time() - t0))


if __name__ == "__main__":
    main()
