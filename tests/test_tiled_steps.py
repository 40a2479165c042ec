"""The row-tiled mode's schedules are planned once (csrc/pm_tiled_steps.hpp::plan_tiled) and both drivers execute the steps.

On the CPU: the plan itself -- tests/cpp/tiled_steps_main.cpp under the sanitizers, and the same list through the C ABI
(pm_tiled_steps) as python/tiled.py reads it.
On the GPU: neither driver enqueues anything else, or in another order, than before the schedules were planned.
tests/golden/tiled_traces.npz (tools/record_tiled_traces.py, cases and recorders in tests/tiled_traces.py) holds, from the
build before that change, the audit log of pm_tiled_run record for record and the comm / tile_* calls of
python/tiled.py::match_band per rank.  The RCCL path cannot run on one GPU: DistComm is held by
test_tiled.py::test_dist_comm_protocol_gloo, and match_band makes the same calls on it as on the LocalComm recorded here.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tiled_traces as T
from conftest import GOLDEN, assert_same

TAKES = (5, 6, 10)   # PRESWEEP, EXCHANGE_ROUND, SET_ROW


# ---- the plan on a host alone ------------------------------------------------------------------------------------------
def test_the_plan_compiles_without_hip_and_is_exact_under_the_sanitizers(tmp_path):
    """tests/cpp/tiled_steps_main.cpp: csrc/pm_tiled_steps.hpp through g++ (no HIP header in reach) with AddressSanitizer and
    UBSan, 1..9 bands, 1..3 iterations, both schedules, every round count: publish before take, no buffer reused unread,
    the exchange counts, who asks ROW_MOVED, and the symbolic run that shows which plans are exact."""
    from cpp_build import build_host_kernel
    exe = build_host_kernel(tmp_path / "tiled_steps_main", "tiled_steps_main.cpp", compiler=("g++",),
                            flags=("-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.endswith(" 0 broken\n"), (r.stdout, r.stderr)


@pytest.mark.parametrize("n", range(1, 10))
def test_the_steps_through_the_c_abi(pm, n):
    """pm_tiled_steps as the Python driver reads it: the same properties on the list that crossed the ABI (so the struct
    layout of the binding is the header's), for every rank's own steps."""
    for iters in (1, 2, 3):
        for schedule in (pm.PM_TILED_SCHEDULE_SPECULATIVE, pm.PM_TILED_SCHEDULE_PIPELINED):
            for rounds in range(n):
                steps = pm.tiled_steps(n, iters, schedule, rounds)
                what = (n, iters, schedule, rounds)
                published = {}   # (band, buffer) -> the band the row is for, until it is taken
                for s in steps:
                    assert 0 <= s.band < n and -1 <= s.iteration < iters and 1 <= s.op <= 10, what
                    if s.op == pm.TILED_PUBLISH:
                        assert published.get((s.band, s.buffer)) is None, what   # not reused before it was read
                        assert s.peer == (s.band + (1 if s.sweep == 1 else -1) if 0 <= s.band + (1 if s.sweep == 1 else -1) < n else -1)
                        published[(s.band, s.buffer)] = s.peer if s.peer >= 0 else None
                    elif s.op in TAKES and s.peer >= 0:
                        assert published.get((s.peer, s.buffer)) == s.band, what   # published, into that buffer, for this band
                        published[(s.peer, s.buffer)] = None
                    elif s.op == pm.TILED_ROW_MOVED:
                        assert 0 <= s.band + (1 if s.sweep == 1 else -1) < n, what   # only a band with a successor asks
                assert not any(v is not None for v in published.values()), what
                taken = sum(1 for s in steps if s.op in TAKES and s.peer >= 0)
                ops = {s.op for s in steps}
                if schedule == pm.PM_TILED_SCHEDULE_PIPELINED:
                    assert taken == 2 * iters * (n - 1), what
                    assert not ops & {pm.TILED_PRESWEEP, pm.TILED_EXCHANGE_ROUND, pm.TILED_ROW_MOVED}, what
                else:
                    assert taken == 2 * iters * ((n - 1) + sum(n - 1 - r for r in range(rounds))), what
                    assert pm.TILED_SET_ROW not in ops, what


def test_the_steps_entry_point_checks_its_arguments(pm):
    lib, total = pm.load(), C.c_int(-1)
    assert lib.pm_tiled_steps(3, 2, 0, -1, None, 0, C.byref(total)) == pm.PM_OK and total.value > 0
    few = (pm.PmTiledStep * 2)()
    assert lib.pm_tiled_steps(3, 2, 0, -1, few, 2, None) == pm.PM_OK and [s.op for s in few] == [pm.TILED_BEGIN] * 2
    for bad in ((0, 2, 0), (3, -1, 0), (3, pm.PM_MAX_ITERS + 1, 0), (3, 2, 2), (3, 2, -1)):
        assert lib.pm_tiled_steps(*bad, -1, None, 0, C.byref(total)) == pm.PM_ERR_INVALID_ARG, bad
    assert lib.pm_tiled_steps(3, 2, 0, -1, few, -1, None) == pm.PM_ERR_INVALID_ARG
    # a negative or too large round count is the exact one; the pipelined schedule has no rounds
    assert len(pm.tiled_steps(4, 2, 0, -1)) == len(pm.tiled_steps(4, 2, 0, 3)) == len(pm.tiled_steps(4, 2, 0, 1 << 20))
    assert len(pm.tiled_steps(4, 2, 1, 0)) == len(pm.tiled_steps(4, 2, 1, 3))


# ---- what the drivers enqueue, against the build before the schedules were planned ------------------------------------
@pytest.fixture(scope="module")
def recorded():
    return T.unpack(np.load(os.path.join(GOLDEN, "tiled_traces.npz")))


@pytest.fixture(scope="module")
def scene(pm, synth):
    images = T.pair(synth)
    with pm.Engine(T.params(pm), max_rows=T.ROWS, max_cols=T.COLS) as e:
        return images, e.match(*images)


def _same_sequence(got, want, what, names):
    if got.shape == want.shape and np.array_equal(got, want):
        return
    n = min(len(got), len(want))
    first = next((i for i in range(n) if not np.array_equal(got[i], want[i])), n)
    show = lambda a: [dict(zip(names, map(int, r))) for r in a[max(first - 2, 0):first + 2]]
    raise AssertionError(f"{what}: {len(got)} records against {len(want)} recorded, first difference at {first}:\n"
                         f"  now      {show(got)}\n  recorded {show(want)}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", T.AUDIT_CASES, ids=T.audit_id)
def test_the_c_driver_makes_the_recorded_runtime_calls(pm, scene, recorded, case):
    """The audit log of pm_tiled_match_u8 on logical devices, without the SET_DEVICE records: every launch, copy, memset,
    event record, wait and synchronisation, with the devices involved, in the recorded order; pm_tiled_info as recorded; no
    violation (but the injected ones, as many as recorded); both maps equal to the untiled Match()."""
    images, (ul, ur) = scene
    logs, infos, bad, maps = T.audit_trace(pm, images, case)
    name = "audit/" + T.audit_id(case)
    for m, (log, info, violations, (dl, dr)) in enumerate(zip(logs, infos, bad, maps)):
        _same_sequence(log, recorded[f"{name}/{m}"], f"{T.audit_id(case)}, match {m}", T.AUDIT_FIELDS)
        assert list(info) + [violations] == recorded[name + "/info"][m].tolist()
        assert violations == 0 or case["inject"]
        assert_same(dl, ul, "tiled vs untiled (left)")
        assert_same(dr, ur, "tiled vs untiled (right)")
    assert len(logs) == case["matches"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", T.DRIVER_CASES, ids=T.driver_id)
def test_the_python_driver_makes_the_recorded_calls(pm, scene, recorded, case):
    """match_tiled_local with recording proxies in place of LocalComm and the engine: every rank's shift(down, send, recv) /
    send(dst, down) / recv(src, down) / any() and tile_*(integers) calls, in the recorded order."""
    import tiled
    images, (ul, ur) = scene
    ranks, dl, dr, info = T.driver_trace(pm, tiled, images, case)
    name = "driver/" + T.driver_id(case)
    for k, calls in enumerate(ranks):
        _same_sequence(calls, recorded[f"{name}/{k}"], f"{T.driver_id(case)}, rank {k}", ("call",) + tuple("abcdefg"))
    assert [info["rounds"], int(info["repeated"]), info["exchanges_per_rank"]] == recorded[name + "/info"][0].tolist()
    assert_same(dl, ul, "tiled vs untiled (left)")
    assert_same(dr, ur, "tiled vs untiled (right)")
