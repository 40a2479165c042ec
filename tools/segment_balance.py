"""How long is the slowest chain of every sweep launch of the headline Match when a chain's segment boundaries are placed
by predicted stops instead of at equal lengths?  CPU only, no device: the oracle driven stage by stage (tests/oracle_lib.py).
Needs the built library all the same (`make`): the plan of every sweep and the boundary rule are taken from its host-only
exports pm_debug_sweep_plan and pm_debug_segment_bounds, so that what is simulated is the rule as shipped.

Per iteration the noise is added (oracle.cpu_add_noise) and the four sweeps run one at a time (oracle.cpu_propagate with
pass_mask = 1 << k) on the left view.  Position p of a chain PASSES iff new[p] == new[p - 1]; any other position is a stop.
A group's steps over a segment follow tools/run_structure.py::steps_of (one candidate per step, nd positions per step, a
stop ends the step).  Group width and wavefronts per chain come from the host-side plan (pm_debug_sweep_plan, no device).
Three ways to cut a chain into its segments:
    equal   the equal split,
    pred    csrc/pm_seg_bounds.hpp::segment_bounds (through pm_debug_segment_bounds) on a PREDICTION of the stops --
            per sweep class `prev` (the stop bits of the same sweep one iteration earlier), `runs` (run boundaries of the
            state the sweep starts from, d0[p] != d0[p - 1]) or `none`,
    true    the same rule on the stops the sweep really has: a bound, not buildable.
Reported per iteration and sweep: slowest and median chain (round-1 steps of the chain's slowest segment) and the mean over
chains of the wave-steps (sum over wavefronts of their slowest group: what the vector units issue); then the sums over the
32 sweeps.  No fix-up rounds, no binade or invalid-candidate stops; a new noise seed per iteration.

    python tools/segment_balance.py [--pair 0] [--chains 128] [--pred prev,none,runs,runs] [--weight 0] [--min-seg 8]
                                    [--snap 0] [--iters 8] [--out file]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import oracle_lib as O
import pm_ctypes as pm
import synth

NAMES = ["row+", "col+", "row-", "col-"]


def steps_of(pass_, lo, hi, cap):
    """tools/run_structure.py::steps_of, one candidate per step"""
    i, n = lo, 0
    while i < hi:
        end = min(hi, i + cap)
        j = i
        while j < end and pass_[j]:
            j += 1
        if j < end:
            j += 1
        i = j
        n += 1
    return n


def bounds(flags, n, nseg, weight, min_len, snap):
    """segment_bounds with a free stop weight and minimum length, and boundaries snapped to the nearest predicted stop within
    `snap` positions (0: none); with the defaults it IS the header function (asserted by the caller)"""
    seg_len = max(-(-n // nseg), min_len)
    if flags is None or not flags.any() or n < nseg * min_len:
        return [min(n, s * seg_len) for s in range(nseg)] + [n]
    prefix = np.concatenate(([0], np.cumsum(np.where(flags != 0, weight, 1))))
    total = int(prefix[-1])
    stops = np.flatnonzero(flags)
    b = [0]
    for s in range(1, nseg):
        j = int(np.searchsorted(prefix, -(-s * total // nseg), side="left"))
        if snap > 0:
            near = stops[np.abs(stops - j) <= snap]
            if len(near):
                j = int(near[np.argmin(np.abs(near - j))])   # the segment starts AT the stop
        b.append(max(j, b[-1] + min_len))
    b.append(n)
    for s in range(nseg - 1, 0, -1):
        b[s] = min(b[s], n - (nseg - s) * min_len)
    return b


def chain_cost(pass_, b, cap, per_wave):
    st = [steps_of(pass_, b[s], b[s + 1], cap) for s in range(len(b) - 1)]
    waves = [max(st[i:i + per_wave]) for i in range(0, len(st), per_wave)]
    return max(st), sum(waves)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pair", type=int, default=0)
    ap.add_argument("--chains", type=int, default=128, help="chains sampled per sweep")
    ap.add_argument("--pred", default="prev,none,runs,runs", help="predictor of row+1, col+1, row-1, col-1: prev / runs / none")
    ap.add_argument("--weight", type=int, default=0, help="what a predicted stop weighs; 0: nd, the positions of a step")
    ap.add_argument("--min-seg", type=int, default=pm.MIN_SEG_LEN)
    ap.add_argument("--snap", type=int, default=0, help="snap a boundary to the nearest predicted stop within this distance")
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--patch", type=int, default=11)
    ap.add_argument("--rows", type=int, default=720)
    ap.add_argument("--cols", type=int, default=1280)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pred = a.pred.split(",")
    assert len(pred) == 4 and all(p in ("prev", "runs", "none") for p in pred)
    O.load()
    rows, cols, pw = a.rows, a.cols, a.patch
    p = synth.make_pair(a.pair, rows, cols)
    ims = O.ImageSet(p["left"], p["right"])
    prm = pm.default_params(0, patch=pw, patchmatch_iters=a.iters)
    d = np.array(p["seed_l"], np.float32)
    h = pw // 2
    lines = [f"# pair {a.pair}, {cols}x{rows}, window {pw}, left view, {a.chains} chains per sweep; predictors {a.pred}; a predicted "
             f"stop weighs {a.weight or 'nd'}, segments of at least {a.min_seg}, snap {a.snap}",
             "it sweep gs nseg nd | slowest chain: equal / pred / true | median chain: equal / pred / true | "
             "mean wave-steps per chain: equal / pred / true"]
    prev_stops = [None] * 4
    tot = np.zeros(3)
    tot_class = np.zeros((4, 3))
    work = np.zeros(3)
    for it in range(a.iters):
        d = O.cpu_add_noise(d, float(prm.noise_amp[it]), mask=d > 0, seed=123 + it)
        for k in range(4):
            before = d
            d = O.cpu_propagate(ims, before, pw, pw, pass_mask=1 << k, nthreads=a.threads)
            axis, dr = k % 2, 1 if k < 2 else -1
            rec = pm.sweep_plan(prm, rows, cols, pw, pw, k, 2, float(prm.noise_amp[it]))
            gs, nseg = rec["group"], (64 // rec["group"]) * rec["waves"]
            nd = gs - pw + (1 if axis == 1 else 0)
            b0, n1 = (before, d) if axis == 0 else (before.T, d.T)
            if dr < 0:
                b0, n1 = b0[:, ::-1], n1[:, ::-1]
            # interior chains, the pixel before the chain in front: index 0
            b0, n1 = b0[h:b0.shape[0] - h, h - 1:b0.shape[1] - h], n1[h:n1.shape[0] - h, h - 1:n1.shape[1] - h]
            nch, n = b0.shape[0], b0.shape[1] - 1
            assert (n, nch) == (rec["chain_len"], rec["chains"])
            stops_true = (n1[:, 1:] != n1[:, :-1]).astype(np.uint8)
            stops_runs = (b0[:, 1:] != b0[:, :-1]).astype(np.uint8)
            guess = {"prev": prev_stops[k], "runs": stops_runs, "none": None}[pred[k]]
            prev_stops[k] = stops_true
            res = np.zeros((a.chains, 3, 2))
            for i, c in enumerate(np.linspace(0, nch - 1, a.chains).astype(int)):
                pass_ = stops_true[c] == 0
                weight = a.weight or nd
                cuts = [bounds(None, n, nseg, weight, a.min_seg, 0),
                        bounds(None if guess is None else guess[c], n, nseg, weight, a.min_seg, a.snap),
                        bounds(stops_true[c], n, nseg, weight, a.min_seg, a.snap)]
                if not a.weight and a.min_seg == pm.MIN_SEG_LEN and not a.snap and i % 16 == 0:   # the shipped rule, itself
                    assert cuts[1] == pm.segment_bounds(None if guess is None else guess[c], n, nseg, nd)
                for m in range(3):
                    res[i, m] = chain_cost(pass_, cuts[m], nd, 64 // gs)
            slow, med, wsteps = res[:, :, 0].max(0), np.median(res[:, :, 0], 0), res[:, :, 1].mean(0)
            tot += slow
            tot_class[k] += slow
            work += wsteps
            f3 = lambda v: " / ".join("%6.1f" % x for x in v)
            lines.append(f"{it} {NAMES[k]} {gs:2d} {nseg:2d} {nd:2d} | {f3(slow)} | {f3(med)} | {f3(wsteps)}")
    lines.append(f"# sum over the {4 * a.iters} sweeps of the launch's slowest chain, round-1 steps: equal {tot[0]:.0f}, pred {tot[1]:.0f}, "
                 f"true {tot[2]:.0f}")
    for k in range(4):
        lines.append(f"#   {NAMES[k]} ({pred[k]}): equal {tot_class[k][0]:.0f}, pred {tot_class[k][1]:.0f}, true {tot_class[k][2]:.0f}")
    lines.append(f"# sum of the mean wave-steps per chain: equal {work[0]:.0f}, pred {work[1]:.0f}, true {work[2]:.0f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
