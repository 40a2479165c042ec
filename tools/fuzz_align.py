"""Differential fuzz of pm_align_evaluate and pm_align_disparity (through the C ABI) against the CPU definition
(tests/align_ref.py).  Random maps <= 40x200 whose rows cross the 64-pixel chunk or not, model and new maps from noise about one
range, from constants and with every special value (0, -0.0, negatives, NaN, +inf, subnormals), normals that are random, constant,
zero, NaN or infinite, motions from none to one that throws the whole map out of the image or behind the camera, options
(min_disp, max_diff, huber_px), source alignments and every subset of the four outputs.  Tolerance 0: the record's 240 bytes on
the device and on the host, the class plane and the residual plane bit-exact, guard bands around every output intact, or it prints
the case and exits 1.  check_align is what tests/test_align.py runs its fixed cases through.

    python tools/fuzz_align.py [--cases 60] [--seed 1]
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import align_ref as AR
from fuzz_cloud import Guarded, SPECIALS, bits, random_disp  # noqa: F401  (re-exported to the tests)
from fuzz_reproject import IDENTITY, random_motion, rotation  # noqa: F401

OUTPUTS = ("class", "residual", "d_sums", "sums")
NORMAL_SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, 3e38], np.float32)


def random_normals(rng, rows, cols, special=0.05):
    """Unit normals about (0, 0, -1) with `special` of the pixels' components drawn from NORMAL_SPECIALS, some pixels all zero."""
    n = rng.normal(0, 0.4, (rows, cols, 3)) + np.array([0.0, 0.0, -1.0])
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    pick = rng.random((rows, cols, 3)) < special
    n[pick] = rng.choice(NORMAL_SPECIALS, int(pick.sum()))
    n[rng.random((rows, cols)) < special] = 0.0
    return n


def check_align(torch, e, camera, opt, motion, disp_model, normals_model, disp_new, outputs=OUTPUTS, offset_floats=0, want=None):
    """One pm_align_evaluate call against the definition.  outputs: which of the four are asked for; offset_floats: the three
    inputs and the residual plane start that many floats past a 16-byte boundary, the class plane that many bytes.  Returns the
    definition's dict."""
    import pm_ctypes as pm
    rows, cols = disp_model.shape
    if want is None:
        want = AR.evaluate(camera, opt, motion, disp_model, normals_model, disp_new)
    off = 4 * offset_floats

    def up(a):
        a = np.ascontiguousarray(a, np.float32).ravel()
        t = torch.zeros(a.size + offset_floats, dtype=torch.float32, device="cuda")
        t[offset_floats:] = torch.from_numpy(a)
        return t

    dm, nm, dn = up(disp_model), up(normals_model), up(disp_new)
    cls = Guarded(torch, rows * cols, offset_floats) if "class" in outputs else None
    res = Guarded(torch, 4 * rows * cols, off) if "residual" in outputs else None
    dev = Guarded(torch, 240) if "d_sums" in outputs else None
    torch.cuda.synchronize()  # the uploads run on torch's stream, the stage on the handle's: nothing else orders them
    sums = e.align_evaluate(camera, dm.data_ptr() + off, nm.data_ptr() + off, dn.data_ptr() + off, rows, cols, motion, opt,
                            cls.ptr if cls else None, res.ptr if res else None, dev.ptr if dev else None, "sums" in outputs)
    e.synchronize()
    record = AR.record(want)
    names = ["H[%d]" % i for i in range(21)] + ["g[%d]" % i for i in range(6)] + ["rr", "n_model / n_gate", "n_used / pad"]

    def same_record(got, where):
        bad = np.flatnonzero(got.view(np.uint64) != record.view(np.uint64))
        assert len(bad) == 0, "pm_align_evaluate: the %s record differs in %s; (got, want): %s" % (
            where, [names[i] for i in bad[:6]], [(got.view(np.float64)[i], record.view(np.float64)[i]) for i in bad[:6]])

    if "sums" in outputs:
        same_record(np.frombuffer(bytes(sums), np.uint8), "host")
    else:
        assert sums is None
    if dev:
        same_record(dev.read(np.uint8), "device")
    if cls:
        got = cls.read(np.uint8).reshape(rows, cols)
        bad = np.argwhere(got != want["cls"])
        assert len(bad) == 0, "pm_align_evaluate: %d of %d classes differ; (y, x, got, want): %s" % (
            len(bad), got.size, [(int(y), int(x), int(got[y, x]), int(want["cls"][y, x])) for y, x in bad[:6]])
    if res:
        got = res.read(np.float32).reshape(rows, cols)
        bad = np.argwhere(bits(got) != bits(want["residual"]))
        assert len(bad) == 0, "pm_align_evaluate: %d of %d residuals differ; (y, x, got, want): %s" % (
            len(bad), got.size, [(int(y), int(x), float(got[y, x]), float(want["residual"][y, x])) for y, x in bad[:6]])
    for t, a, name in ((dm, disp_model, "d_disp_model"), (nm, normals_model, "d_normals_model"), (dn, disp_new, "d_disp_new")):
        assert np.array_equal(bits(t.cpu().numpy()[offset_floats:]), bits(np.asarray(a, np.float32)).ravel()), "pm_align_evaluate wrote to " + name
    return want


def check_align_disparity(torch, e, camera, opt, guess, disp_model, normals_model, disp_new, want=None):
    """One pm_align_disparity call against the definition: the motion, the info and H bit for bit.  Returns (motion, info)."""
    rows, cols = disp_model.shape
    if want is None:
        want = AR.align(camera, opt, guess, disp_model, normals_model, disp_new)
    dm, nm, dn = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (disp_model, normals_model, disp_new))
    torch.cuda.synchronize()
    R, t, info = e.align_disparity(camera, dm.data_ptr(), nm.data_ptr(), dn.data_ptr(), rows, cols, guess, opt)
    (wR, wt), winfo = want
    assert np.array_equal(R.view(np.uint64), wR.view(np.uint64)) and np.array_equal(t.view(np.uint64), wt.view(np.uint64)), (R, t, wR, wt)
    for k in ("valid", "n_model", "n_gate", "n_used", "iterations"):
        assert info[k] == winfo[k], (k, info[k], winfo[k])
    assert np.float64(info["rms_px"]).view(np.uint64) == np.float64(winfo["rms_px"]).view(np.uint64), (info["rms_px"], winfo["rms_px"])
    assert np.array_equal(info["H"].view(np.uint64), np.asarray(winfo["H"], np.float64).view(np.uint64))
    return want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=60)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import torch
    import pm_ctypes as pm
    rng = np.random.default_rng(a.seed)
    t0, totals = time.time(), np.zeros(3, np.int64)
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        for case in range(a.cases):
            rows, cols = int(rng.integers(1, 41)), int(rng.choice([1, 7, 63, 64, 65, 130, 200]))
            f = float(rng.uniform(0.6, 2.0) * max(cols, 16))
            camera = (f, f * float(rng.uniform(0.8, 1.25)), cols / 2 + float(rng.normal(0, 2)), rows / 2 + float(rng.normal(0, 2)),
                      float(rng.uniform(0.05, 0.3)))
            depth = float(rng.uniform(0.5, 4.0))
            mid = camera[0] * camera[4] / depth
            kind, motion = random_motion(rng, camera, depth)
            special = float(rng.choice([0.0, 0.1]))
            dm = random_disp(rng, rows, cols, valid=float(rng.choice([0.6, 1.0])), special=special, lo=0.9 * mid, hi=1.1 * mid)
            dn = random_disp(rng, rows, cols, valid=float(rng.choice([0.6, 1.0])), special=special, lo=0.9 * mid, hi=1.1 * mid)
            if rng.random() < 0.3:
                dm[dm > 0] = np.float32(mid)
                dn[dn > 0] = np.float32(mid)
            nm = random_normals(rng, rows, cols, special=special / 2)
            opt = AR.options(min_disp=float(rng.choice([0.0, 0.95 * mid])), max_diff=float(rng.choice([0.0, 0.05, 0.3, 10.0]) * mid),
                             huber_px=float(rng.choice([0.05, 1.0, 1e6])))
            outputs = tuple(k for k in OUTPUTS if rng.random() < 0.7) or ("sums",)
            what = dict(case=case, rows=rows, cols=cols, camera=camera, motion=kind, opt=opt, outputs=outputs)
            try:
                want = check_align(torch, e, camera, opt, motion, dm, nm, dn, outputs, int(rng.integers(0, 4)))
                totals += (want["n_model"], want["n_gate"], want["n_used"])
                if case % 10 == 0:
                    check_align_disparity(torch, e, camera, AR.options(**dict(opt, iterations=3, min_used=6)), motion, dm, nm, dn)
            except AssertionError as err:
                print("MISMATCH", what, err)
                sys.exit(1)
    print("fuzz_align: %d cases (seed %d), %d model pixels, %d at the gate, %d used, bit-identical to the definition, %.1f s"
          % (a.cases, a.seed, *totals, time.time() - t0))


if __name__ == "__main__":
    main()
