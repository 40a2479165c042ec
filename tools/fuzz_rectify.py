"""Differential fuzz of the rectification kernels: pm_rectify_u8, its mask and pm_rectify_map (through the C ABI) against
the CPU definition (tests/rectify_ref.py); with --bgr pm_rectify_bgr8 (8-bit image, float image, mask, each optional)
against tests/rectify_bgr_ref.py.  Random source / destination sizes, strides, image counts, border values,
destination alignments, camera models (mild to absurd distortion), rotations (small, large, past 90 degrees) and new
pinholes.  Tolerance 0: bit-exact or it prints the case and exits 1.

    python tools/fuzz_rectify.py [--bgr] [--cases 40] [--seed 1] [--max-rows 200] [--max-cols 300]
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import rectify_ref as RR


def rotation(rng, max_deg):
    w = rng.normal(size=3)
    w *= np.deg2rad(rng.uniform(0, max_deg)) / np.linalg.norm(w)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def random_view(rng, src_rows, src_cols, rows, cols):
    kind = rng.choice(["mild", "strong", "absurd", "identity"], p=[0.45, 0.3, 0.15, 0.1])
    f = float(rng.uniform(0.4, 2.0) * src_cols)
    cam = [f, f * float(rng.uniform(0.9, 1.1)), src_cols / 2 + float(rng.normal(0, 3)), src_rows / 2 + float(rng.normal(0, 3)),
           0, 0, 0, 0, 0]
    if kind == "mild":
        cam[4:] = [rng.uniform(-0.3, 0.1), rng.uniform(-0.1, 0.1), rng.normal(0, 1e-3), rng.normal(0, 1e-3), rng.uniform(-0.02, 0.02)]
    elif kind == "strong":
        cam[4:] = [rng.uniform(-2, 2), rng.uniform(-3, 3), rng.normal(0, 0.05), rng.normal(0, 0.05), rng.uniform(-5, 5)]
    elif kind == "absurd":  # positions far outside the image, past 2^30 in Q5, overflow to inf
        cam[4:] = [rng.uniform(-1, 1) * 10.0 ** rng.integers(0, 300) for _ in range(5)]
    if kind == "identity":
        return kind, RR.make_view(cam, np.eye(3), cam[:4])
    R = rotation(rng, float(rng.choice([3.0, 30.0, 120.0, 180.0])))
    fn = f * float(rng.uniform(0.5, 1.5)) * cols / src_cols
    pin = [fn * float(rng.choice([1.0, -1.0], p=[0.9, 0.1])), fn * float(rng.uniform(0.9, 1.1)),
           cols / 2 + float(rng.normal(0, 5)), rows / 2 + float(rng.normal(0, 5))]
    return kind, RR.make_view(cam, R, pin)


def fuzz_bgr(a, pm, torch):
    """pm_rectify_bgr8.  Its own draw sequence: the gray mode's stays what it was."""
    import rectify_bgr_ref as RB
    rng = np.random.default_rng(a.seed)
    t0 = time.time()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        side = torch.cuda.Stream()
        for case in range(a.cases):
            src_rows, src_cols = int(rng.integers(1, a.max_rows + 1)), int(rng.integers(1, a.max_cols + 1))
            if rng.integers(0, 8) == 0:
                src_cols = int(rng.integers(1, 3))  # one or two columns: no 6-byte window, or exactly one
            rows, cols = int(rng.integers(1, a.max_rows + 1)), int(rng.integers(1, a.max_cols + 1))
            n = int(rng.choice([1, 1, 2, 3]))
            step = 3 * src_cols + int(rng.choice([0, 0, 1, 5, 64]))  # bytes
            border = int(rng.choice([0, 255, rng.integers(0, 256)]))
            shift = int(rng.integers(0, 4))  # the 8-bit image and the mask start `shift` bytes in, the float image 4 * shift
            own_stream = bool(rng.integers(0, 2))
            outs = int(rng.choice([1, 2, 3, 5, 6, 7, 7, 7]))  # bit 0: 8-bit image, bit 1: float image, bit 2: mask
            pass_zero_step = step == 3 * src_cols and bool(rng.integers(0, 2))
            kind, view = random_view(rng, src_rows, src_cols, rows, cols)
            raw = rng.integers(0, 256, (n, src_rows, step), dtype=np.uint8)
            want, want_f, want_valid, want_xy = RB.rectify_bgr(raw[:, :, :3 * src_cols].reshape(n, src_rows, src_cols, 3), view,
                                                               rows, cols, border)
            d_src = torch.from_numpy(raw).cuda()
            total = n * rows * cols
            bufs = [torch.full((size + 32,), 0xA5, dtype=torch.uint8, device="cuda") for size in (3 * total, 12 * total, total)]
            offs = (shift, 4 * shift, shift)
            wants = (want, want_f.view(np.uint8), want_valid)
            torch.cuda.synchronize()  # the fills above ran on torch's stream; the call below runs on another
            ptrs = [b.data_ptr() + o if outs >> k & 1 else None for k, (b, o) in enumerate(zip(bufs, offs))]
            e.rectify_bgr8(view, d_src.data_ptr(), n, src_rows, src_cols, 0 if pass_zero_step else step, rows, cols, border, *ptrs,
                           side.cuda_stream if own_stream else None)
            if own_stream:
                side.synchronize()
            e.synchronize()
            ok = True
            for k, (b, o, w) in enumerate(zip(bufs, offs, wants)):
                got = b.cpu().numpy()
                if outs >> k & 1:
                    ok = ok and np.array_equal(got[o:o + w.size], w.ravel())
                    ok = ok and (got[:o] == 0xA5).all() and (got[o + w.size:] == 0xA5).all()  # nothing written outside
                else:
                    ok = ok and (got == 0xA5).all()
            print(f"case {case:3d}: {n} x {src_cols}x{src_rows} bgr step {step} -> {cols}x{rows} {kind} border {border} shift {shift} "
                  f"stream {int(own_stream)} outputs {outs} invalid {float((want_xy[:, :, 0] == RR.INVALID).mean()):.2f} "
                  f"valid {float((want_valid == 255).mean()):.2f} {'ok' if ok else 'MISMATCH'}  [{time.time() - t0:.0f} s]", flush=True)
            if not ok:
                print("view:", repr(view.tolist()))
                sys.exit(1)
    print("all", a.cases, "bgr cases bit-identical")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bgr", action="store_true", help="fuzz pm_rectify_bgr8 instead of pm_rectify_u8 / pm_rectify_map")
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-rows", type=int, default=200)
    ap.add_argument("--max-cols", type=int, default=300)
    a = ap.parse_args()
    import pm_ctypes as pm
    pm.load()
    import torch
    if a.bgr:
        return fuzz_bgr(a, pm, torch)
    rng = np.random.default_rng(a.seed)
    t0 = time.time()
    with pm.Engine(pm.default_params(0, patch=5), max_rows=64, max_cols=64) as e:
        side = torch.cuda.Stream()
        for case in range(a.cases):
            src_rows, src_cols = int(rng.integers(1, a.max_rows + 1)), int(rng.integers(1, a.max_cols + 1))
            rows, cols = int(rng.integers(1, a.max_rows + 1)), int(rng.integers(1, a.max_cols + 1))
            n = int(rng.choice([1, 1, 2, 3]))
            step = src_cols + int(rng.choice([0, 0, 1, 5, 64]))
            border = int(rng.choice([0, 255, rng.integers(0, 256)]))
            shift = int(rng.integers(0, 4))  # destination and mask start `shift` bytes into their allocations
            own_stream = bool(rng.integers(0, 2))
            want_mask = bool(rng.integers(0, 4))
            kind, view = random_view(rng, src_rows, src_cols, rows, cols)
            raw = rng.integers(0, 256, (n, src_rows, step), dtype=np.uint8)
            want, want_valid, want_xy = RR.rectify(raw[:, :, :src_cols], view, rows, cols, border)
            d_src = torch.from_numpy(raw).cuda()
            total = n * rows * cols
            d_dst = torch.full((total + 8,), 0xA5, dtype=torch.uint8, device="cuda")
            d_val = torch.full((total + 8,), 0xA5, dtype=torch.uint8, device="cuda")
            d_xy = torch.zeros((rows, cols, 2), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()  # the fills above ran on torch's stream; the calls below run on other streams
            stream = side.cuda_stream if own_stream else None
            e.rectify_u8(view, d_src.data_ptr(), n, src_rows, src_cols, step if step != src_cols or rng.integers(0, 2) else 0, rows,
                         cols, border, d_dst.data_ptr() + shift, d_val.data_ptr() + shift if want_mask else None, stream)
            e.rectify_map(view, rows, cols, d_xy.data_ptr())
            if own_stream:
                side.synchronize()
            e.synchronize()
            got, got_val, got_xy = d_dst.cpu().numpy(), d_val.cpu().numpy(), d_xy.cpu().numpy()
            ok = np.array_equal(got[shift:shift + total].reshape(want.shape), want) and np.array_equal(got_xy, want_xy)
            ok = ok and (got[:shift] == 0xA5).all() and (got[shift + total:] == 0xA5).all()  # nothing written outside
            if want_mask:
                ok = ok and np.array_equal(got_val[shift:shift + total].reshape(want.shape), want_valid)
                ok = ok and (got_val[:shift] == 0xA5).all() and (got_val[shift + total:] == 0xA5).all()
            else:
                ok = ok and (got_val == 0xA5).all()
            print(f"case {case:3d}: {n} x {src_cols}x{src_rows} step {step} -> {cols}x{rows} {kind} border {border} shift {shift} "
                  f"stream {int(own_stream)} mask {int(want_mask)} invalid {float((want_xy[:, :, 0] == RR.INVALID).mean()):.2f} "
                  f"valid {float((want_valid == 255).mean()):.2f} {'ok' if ok else 'MISMATCH'}  [{time.time() - t0:.0f} s]", flush=True)
            if not ok:
                print("view:", repr(view.tolist()))
                sys.exit(1)
    print("all", a.cases, "cases bit-identical")


if __name__ == "__main__":
    main()
