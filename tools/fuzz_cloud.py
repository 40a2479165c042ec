"""Differential fuzz of the point-cloud stages: pm_backproject and pm_point_cloud (through the C ABI) against the CPU
definition (tests/pointcloud_ref.py).  Random shapes <= 96x160, disparity maps with every special value (0, -0.0, negatives,
NaN, +inf, subnormals), masks from empty to full, cameras, filters (min_disp, max_range, stride), capacities around the
count, destination alignments and every subset of the optional streams.  Tolerance 0: bit-exact, guard bands around every
output intact, or it prints the case and exits 1.  check_backproject / check_cloud are what tests/test_pointcloud.py runs
its fixed cases through.

    python tools/fuzz_cloud.py [--cases 60] [--seed 1] [--max-rows 96] [--max-cols 160]
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import pointcloud_ref as PR

GUARD = 64    # bytes of 0xA5 on either side of every output (keeps the 16-byte alignment of the allocation)
FILL = 0xA5
SPECIALS = np.array([0.0, -0.0, -1.0, -37.5, np.nan, np.inf, 1e-45, 1e-39, 1.1754942e-38], np.float32)


def bits(a):
    """The bit patterns of an array: -0.0 and +0.0 differ, equal NaNs are equal."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def random_disp(rng, rows, cols, valid=0.6, special=0.1, lo=0.5, hi=90.0):
    """A map with `valid` of its pixels in [lo, hi), `special` of them drawn from SPECIALS, the rest 0."""
    d = rng.uniform(lo, hi, (rows, cols)).astype(np.float32)
    u = rng.random((rows, cols))
    d[u >= valid] = 0.0
    pick = rng.random((rows, cols)) < special
    d[pick] = rng.choice(SPECIALS, int(pick.sum()))
    return d


class Guarded:
    """A device buffer of nbytes behind `offset` bytes, with GUARD bytes of FILL on either side."""

    def __init__(self, torch, nbytes, offset=0):
        self.lo, self.n = GUARD + offset, nbytes
        self.t = torch.full((self.lo + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # the fill runs on torch's stream, the stage on the handle's: nothing else orders them
        self.ptr = self.t.data_ptr() + self.lo

    def read(self, dtype, written=None):
        """The payload as `dtype`; asserts the guards -- and the payload bytes from `written` on -- still hold FILL."""
        a = self.t.cpu().numpy()
        written = self.n if written is None else written
        assert (a[:self.lo] == FILL).all(), "bytes in front of the output were written"
        assert (a[self.lo + written:] == FILL).all(), "bytes behind the last written element were written"
        return a[self.lo:self.lo + written].copy().view(dtype)


def check_backproject(torch, e, disp, camera, offset_floats=0):
    rows, cols = disp.shape
    d = torch.from_numpy(disp).cuda()
    out = Guarded(torch, 12 * rows * cols, 4 * offset_floats)
    e.backproject(camera, d.data_ptr(), rows, cols, out.ptr)
    e.synchronize()
    got = out.read(np.float32).reshape(rows, cols, 3)
    want = PR.backproject(disp, camera)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, "pm_backproject: %d of %d values differ; (y, x, channel, disparity, got, want): %s" % (
        len(bad), got.size, [(int(y), int(x), int(c), float(disp[y, x]), float(got[y, x, c]), float(want[y, x, c]))
                             for y, x, c in bad[:6]])
    return got


def check_cloud(torch, e, disp, camera, min_disp=0.0, max_range=0.0, stride=1, capacity="count", normal_map=None, bgr=None,
                outputs=("xyz", "normals", "bgr", "index"), d_count=True, host_count=True):
    """One pm_point_cloud call against the definition.  capacity: an int, or "count" / "count-1" (of the definition's
    count).  outputs: the optional streams that are asked for.  Returns the definition's count."""
    rows, cols = disp.shape
    want_all = PR.point_cloud(disp, camera, min_disp, max_range, stride, None, normal_map, bgr)
    count = want_all["count"]
    cap = count if capacity == "count" else count - 1 if capacity == "count-1" else int(capacity)
    if cap < 0:
        return count
    m = min(count, cap)
    d = torch.from_numpy(disp).cuda()
    dn = torch.from_numpy(np.ascontiguousarray(normal_map, np.float32)).cuda() if normal_map is not None else None
    dc = torch.from_numpy(np.ascontiguousarray(bgr, np.uint8)).cuda() if bgr is not None else None
    width = {"xyz": 12, "normals": 12, "bgr": 3, "index": 4}
    bufs = {k: Guarded(torch, width[k] * cap) for k in outputs}
    cnt = Guarded(torch, 4) if d_count else None
    ptr = lambda k: bufs[k].ptr if k in bufs else None
    n = e.point_cloud(camera, d.data_ptr(), rows, cols, cap, min_disp, max_range, stride,
                      dn.data_ptr() if dn is not None else None, dc.data_ptr() if dc is not None else None, ptr("xyz"),
                      ptr("normals"), ptr("bgr"), ptr("index"), cnt.ptr if cnt else None, host_count)
    e.synchronize()
    if host_count:
        assert n == count, "host count %d, definition %d" % (n, count)
    if cnt:
        assert int(cnt.read(np.int32)[0]) == count, "d_count %d, definition %d" % (int(cnt.read(np.int32)[0]), count)
    dtypes = {"xyz": np.float32, "normals": np.float32, "bgr": np.uint8, "index": np.int32}
    for k, buf in bufs.items():
        got = buf.read(dtypes[k], width[k] * m)  # slots at and beyond min(count, capacity) keep the guard pattern
        want = want_all[k][:m]
        assert np.array_equal(bits(got), bits(want.ravel())), "pm_point_cloud: %s differs" % k
        if k == "index" and m > 1:
            assert (np.diff(got) > 0).all(), "d_index_out is not strictly increasing"
    return count


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
    t0, points = time.time(), 0
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        for case in range(a.cases):
            rows, cols = int(rng.integers(1, a.max_rows + 1)), int(rng.integers(1, a.max_cols + 1))
            f = float(rng.uniform(0.4, 2.0) * cols)
            camera = (f * float(rng.choice([1.0, -1.0], p=[0.9, 0.1])), f * float(rng.uniform(0.8, 1.25)),
                      cols / 2 + float(rng.normal(0, 3)), rows / 2 + float(rng.normal(0, 3)), float(rng.uniform(0.02, 0.5)))
            disp = random_disp(rng, rows, cols, valid=float(rng.choice([0.0, 0.05, 0.5, 0.95, 1.0])),
                               special=float(rng.choice([0.0, 0.1, 0.5])))
            kw = dict(min_disp=float(rng.choice([0.0, 0.0, 5.0, 45.0, np.inf])),
                      max_range=float(rng.choice([0.0, 0.0, f * 0.1 / 20.0, 1e-3, 1e30])),
                      stride=int(rng.choice([1, 1, 2, 3, 7, 200])),
                      capacity=rng.choice(["count", "count-1", "0", "1", "5", "100000"]))
            if kw["capacity"] not in ("count", "count-1"):
                kw["capacity"] = int(kw["capacity"])
            outputs = tuple(k for k in ("xyz", "normals", "bgr", "index") if rng.random() < 0.7)
            normal_map = rng.normal(size=(rows, cols, 3)).astype(np.float32) if "normals" in outputs or rng.random() < 0.3 else None
            bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8) if "bgr" in outputs or rng.random() < 0.3 else None
            what = dict(case=case, rows=rows, cols=cols, camera=camera, outputs=outputs, **kw)
            try:
                check_backproject(torch, e, disp, camera, int(rng.integers(0, 4)))
                points += check_cloud(torch, e, disp, camera, normal_map=normal_map, bgr=bgr, outputs=outputs,
                                      d_count=bool(rng.random() < 0.7), host_count=bool(rng.random() < 0.7), **kw)
            except AssertionError as err:
                print("MISMATCH", what, err)
                sys.exit(1)
    print("fuzz_cloud: %d cases (seed %d), %d points counted, bit-identical to the definition, %.1f s"
          % (a.cases, a.seed, points, time.time() - t0))


if __name__ == "__main__":
    main()
