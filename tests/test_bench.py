"""bench.py's plain run (set-up, warm-up, timed steps, outputs, one line) against its --full run, and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY_KEYS = ("check", "cpu_baseline", "host_sequence_all_ranks", "host_buffers", "sequence_device", "batch",
                  "reference_test_shape", "tiled_4096x2160", "planes", "run_engine_counters_per_step")


def run_bench(*extra, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(extra), cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    return json.loads(lines[0])


def test_plain_dry_run_prints_the_headline_only():
    out = run_bench("--gpus", "1", "--steps", "3", "--warmup", "0", "--dry-run")
    assert all(k in out for k in HEADLINE_KEYS), out
    assert out["steps"] == 3 and abs(out["value"] - 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    assert not [k for k in FULL_ONLY_KEYS if k in out], out
    full = run_bench("--gpus", "1", "--steps", "3", "--warmup", "0", "--dry-run", "--full", "--host-pairs", "4")
    assert all(k in full for k in HEADLINE_KEYS) and full["host_sequence_all_ranks"]["frames_per_rank"] == 4


def test_dump_outputs_samples_large_maps_within_the_limit(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    import torch

    class Eng:
        def synchronize(self):
            pass

    class W:
        eng = Eng()
        DL = torch.arange(9 * 1000 * 1000, dtype=torch.float32).reshape(9, 1000, 1000)
        DR = -DL

    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), W(), np)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["disparity_left.npy", "disparity_right.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10**6
    left, right = (np.load(tmp_path / "a" / f) for f in files)
    assert left.dtype == np.float32 and left.size == bench.DUMP_LIMIT_BYTES // 8
    assert np.all(np.diff(left) > 0) and np.array_equal(right, -left)  # sorted positions, the same ones in both maps
    for f in files:  # a fixed sample: the same positions in every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_dump_outputs_hold_the_last_timed_steps_maps(tmp_path):
    """A plain run at a small shape: the line carries the headline fields only, and the dumped maps are the last timed
    step's -- step 2 of 3 matches rank 0's resident pair 2 -- bit-identical to the oracle on that pair."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
    import oracle_lib as O
    import synth
    rows, cols, patch, iters = 96, 160, 7, 2
    out = run_bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", str(rows), "--cols", str(cols),
                    "--patch", str(patch), "--iters", str(iters), "--dump-outputs", str(tmp_path))
    assert all(k in out for k in HEADLINE_KEYS) and out["steps"] == 3 and out["value"] > 0, out
    assert not [k for k in FULL_ONLY_KEYS if k in out], out
    dl, dr = np.load(tmp_path / "disparity_left.npy"), np.load(tmp_path / "disparity_right.npy")
    assert dl.dtype == np.float32 and dl.shape == dr.shape == (1, rows, cols)
    p = synth.make_pair(2, rows, cols)
    el, er = O.match(O.default_params(O.SEM_CPU, patch=patch, n_iters=iters, nthreads=4), p["left"], p["right"],
                     p["seed_l"], p["seed_r"])
    assert np.array_equal(dl[0], el) and np.array_equal(dr[0], er)
