"""Differential fuzz of pm_reproject_disparity (through the C ABI) against the CPU definition (tests/reproject_ref.py).
Random shapes <= 96x160, disparity maps with every special value (0, -0.0, negatives, NaN, +inf, subnormals), rigid motions
from none to one that throws the whole map out of the image or behind the camera, options (min_disp, max_disp,
close_radius 0..3), source alignments and every subset of the four outputs.  Tolerance 0: both seed maps and both counts
bit-exact, guard bands around every output intact, or it prints the case and exits 1.  check_reproject is what
tests/test_reproject.py runs its fixed cases through.

    python tools/fuzz_reproject.py [--cases 60] [--seed 1] [--max-rows 96] [--max-cols 160]
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import reproject_ref as RR
from fuzz_cloud import Guarded, SPECIALS, bits, random_disp  # noqa: F401  (re-exported to the tests)

IDENTITY = (np.eye(3).ravel(), np.zeros(3))


def rotation(axis, degrees):
    """Rodrigues: the rotation by `degrees` about `axis` -> 3x3 binary64."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    a = np.deg2rad(np.float64(degrees))
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def check_reproject(torch, e, disp, camera, motion, min_disp=0.0, max_disp=0.0, close_radius=1,
                    outputs=("seed_l", "seed_r", "d_counts", "counts"), offset_floats=0, want=None):
    """One pm_reproject_disparity call against the definition; outputs: which of the four are asked for; offset_floats: the
    source and both maps start that many floats past a 16-byte boundary.  Returns the definition's dict."""
    rows, cols = disp.shape
    if want is None:
        want = RR.reproject(disp, camera, motion[0], motion[1], min_disp, max_disp, close_radius)
    src = torch.zeros(rows * cols + offset_floats, dtype=torch.float32, device="cuda")
    src[offset_floats:] = torch.from_numpy(disp.ravel())
    maps = {k: Guarded(torch, 4 * rows * cols, 4 * offset_floats) for k in ("seed_l", "seed_r") if k in outputs}
    cnt = Guarded(torch, 8) if "d_counts" in outputs else None
    torch.cuda.synchronize()  # the upload runs on torch's stream, the stage on the handle's: nothing else orders them
    n = e.reproject_disparity(camera, motion, src.data_ptr() + 4 * offset_floats, rows, cols, min_disp, max_disp, close_radius,
                              maps["seed_l"].ptr if "seed_l" in maps else None, maps["seed_r"].ptr if "seed_r" in maps else None,
                              cnt.ptr if cnt else None, "counts" in outputs)
    e.synchronize()
    if "counts" in outputs:
        assert tuple(n) == tuple(int(v) for v in want["counts"]), "host counts %s, definition %s" % (n, want["counts"])
    else:
        assert n is None
    if cnt:
        got = cnt.read(np.int32)
        assert np.array_equal(got, want["counts"]), "d_counts %s, definition %s" % (got, want["counts"])
    for k, buf in maps.items():
        got = buf.read(np.float32).reshape(rows, cols)
        bad = np.argwhere(bits(got) != bits(want[k]))
        assert len(bad) == 0, "pm_reproject_disparity: %d of %d values of %s differ; (y, x, got, want): %s" % (
            len(bad), got.size, k, [(int(y), int(x), float(got[y, x]), float(want[k][y, x])) for y, x in bad[:6]])
    return want


def random_motion(rng, camera, depth):
    """A motion of a random kind; `depth`: a typical range of the scene."""
    kind = rng.choice(["identity", "baseline", "advance", "retreat", "yaw", "pitch", "roll", "mixed", "behind", "gone", "huge"])
    R, t = np.eye(3), np.zeros(3)
    if kind == "baseline":
        t = np.array([-camera[4], 0.0, 0.0])
    elif kind == "advance":
        t = np.array([0.0, 0.0, -depth * rng.uniform(0.02, 0.3)])
    elif kind == "retreat":
        t = np.array([0.0, 0.0, depth * rng.uniform(0.02, 0.5)])
    elif kind in ("yaw", "pitch", "roll"):
        axis = {"yaw": (0, 1, 0), "pitch": (1, 0, 0), "roll": (0, 0, 1)}[kind]
        R = rotation(axis, rng.uniform(-6, 6) if kind != "roll" else rng.uniform(-180, 180))
    elif kind == "mixed":
        R = rotation(rng.normal(size=3), rng.uniform(-4, 4))
        t = rng.normal(size=3) * depth * 0.05
    elif kind == "behind":
        t = np.array([0.0, 0.0, -depth * rng.uniform(0.8, 1.5)])
    elif kind == "gone":
        t = np.array([depth * 1e3, 0.0, 0.0])
    elif kind == "huge":  # image coordinates beyond 2^30
        t = np.array([-depth * 1e12, depth * 1e13, 0.0])
    return kind, (R.ravel(), t)


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
    t0, seeds = time.time(), 0
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        for case in range(a.cases):
            rows, cols = int(rng.integers(1, a.max_rows + 1)), int(rng.integers(1, a.max_cols + 1))
            f = float(rng.uniform(0.4, 2.0) * cols)
            camera = (f, f * float(rng.uniform(0.8, 1.25)), cols / 2 + float(rng.normal(0, 3)), rows / 2 + float(rng.normal(0, 3)),
                      float(rng.uniform(0.02, 0.5)))
            hi = float(rng.choice([4.0, 30.0, 90.0]))
            disp = random_disp(rng, rows, cols, valid=float(rng.choice([0.0, 0.05, 0.5, 0.95, 1.0])),
                               special=float(rng.choice([0.0, 0.1, 0.5])), hi=hi)
            if rng.random() < 0.5:  # piecewise constant: surfaces that collide instead of noise
                disp[disp > 0] = np.round(disp[disp > 0] / (hi / 3)) * np.float32(hi / 3) + np.float32(0.5)
            kind, motion = random_motion(rng, camera, camera[0] * camera[4] / (hi / 2))
            kw = dict(min_disp=float(rng.choice([0.0, 0.0, 1.0, hi / 2])), max_disp=float(rng.choice([0.0, 0.0, hi / 2, hi])),
                      close_radius=int(rng.integers(0, 4)))
            outputs = tuple(k for k in ("seed_l", "seed_r", "d_counts", "counts") if rng.random() < 0.7) or ("seed_r",)
            what = dict(case=case, rows=rows, cols=cols, camera=camera, motion=kind, outputs=outputs, **kw)
            try:
                want = check_reproject(torch, e, disp, camera, motion, outputs=outputs, offset_floats=int(rng.integers(0, 4)), **kw)
                seeds += int(want["counts"].sum())
            except AssertionError as err:
                print("MISMATCH", what, err)
                sys.exit(1)
    print("fuzz_reproject: %d cases (seed %d), %d seeds counted, bit-identical to the definition, %.1f s"
          % (a.cases, a.seed, seeds, time.time() - t0))


if __name__ == "__main__":
    main()
