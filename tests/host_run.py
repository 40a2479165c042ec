"""What the tests that run kernel code on the host (tests/cpp/*_host_main.cpp) share on the Python side: writing a case as
the directory of .npy dumps that tests/cpp/host_npy.hpp reads, and showing that a program does compare."""
import os
import subprocess

import numpy as np


def dump_case(path, params, **arrays):
    """Creates directory `path` and writes params.npy (float64) and <name>.npy, C-contiguous, for every array given."""
    os.makedirs(path)
    for name, a in dict(arrays, params=np.array(params, np.float64)).items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))


def flat_motions(mots, slots):
    """`slots` x (R[9], t[3]) as one flat float64 list, the motions of `mots` in front and zeros behind them."""
    flat = np.zeros(12 * slots)
    for k, (R, t) in enumerate(mots):
        flat[12 * k:12 * k + 12] = [*np.asarray(R).ravel(), *np.asarray(t).ravel()]
    return flat


def assert_program_compares(exe, case_dir, dumps):
    """One flipped bit in an expectation is a mismatch, not a pass.  For every (dump name, dtype, words) of `dumps`: with the
    lowest bit of the dump's last element flipped the program ends with status 1 and `words` on stderr; with the dump put back,
    at the end, with status 0."""
    for name, dtype, words in dumps:
        path = os.path.join(case_dir, name + ".npy")
        keep = np.load(path)
        flipped = keep.copy()
        flipped.view(dtype).ravel()[-1] ^= 1
        np.save(path, flipped)
        r = subprocess.run([exe, case_dir], capture_output=True, text=True)
        assert r.returncode == 1 and words in r.stderr, (name, r.returncode, r.stderr[-500:])
        np.save(path, keep)
    assert subprocess.run([exe, case_dir], capture_output=True, text=True).returncode == 0
