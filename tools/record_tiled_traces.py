#!/usr/bin/env python3
"""Records what the row-tiled drivers enqueue into tests/golden/tiled_traces.npz (needs a GPU).

    python tools/record_tiled_traces.py [--out tests/golden/tiled_traces.npz]

Run it on the commit whose behaviour is to be kept -- before a change of csrc/pm_tiled.hip or python/tiled.py that must not
move a launch, a copy, an event or a wait -- and commit the file; tests/test_tiled_steps.py then holds every later build to
it.  Cases and recorders: tests/tiled_traces.py.  Every recorded match is also checked against the untiled Match() here, so
that a fixture is never taken from a driver that computes something else.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "tiled_traces.npz"))
    args = ap.parse_args()
    import pm_ctypes as pm
    import synth
    import tiled
    import tiled_traces as T
    images = T.pair(synth)
    with pm.Engine(T.params(pm), max_rows=T.ROWS, max_cols=T.COLS) as e:
        ul, ur = e.match(*images)
    out = {}
    for c in T.AUDIT_CASES:
        logs, infos, bad, maps = T.audit_trace(pm, images, c)
        for dl, dr in maps:
            assert np.array_equal(dl, ul) and np.array_equal(dr, ur), T.audit_id(c)
        assert all(b == 0 for b in bad) or c["inject"], (T.audit_id(c), bad)
        for m, log in enumerate(logs):
            out["audit/%s/%d" % (T.audit_id(c), m)] = log
        out["audit/%s/info" % T.audit_id(c)] = np.array([list(i) + [b] for i, b in zip(infos, bad)], np.int32)
        print(T.audit_id(c), [len(l) for l in logs], infos, bad, flush=True)
    for c in T.DRIVER_CASES:
        ranks, dl, dr, info = T.driver_trace(pm, tiled, images, c)
        assert np.array_equal(dl, ul) and np.array_equal(dr, ur), T.driver_id(c)
        for k, calls in enumerate(ranks):
            out["driver/%s/%d" % (T.driver_id(c), k)] = calls
        out["driver/%s/info" % T.driver_id(c)] = np.array([[info["rounds"], int(info["repeated"]),
                                                             info["exchanges_per_rank"]]], np.int32)
        print(T.driver_id(c), [len(r) for r in ranks], info, flush=True)
    np.savez_compressed(args.out, **T.pack(out))
    print("wrote %s: %d traces, %d bytes" % (args.out, len(out), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
