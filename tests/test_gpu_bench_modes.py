"""bench.py's multi-GPU layouts at world size 1 (RCCL communicator of one rank), as a child
process: the partitioned (route -> grouped send/recv -> owner ops -> packed answers ->
combine) and replicated (gather / OR-all-reduce insert) steps run end to end, every step's
members are found (bench.py asserts it), and the JSON line keeps the driver's contract."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode,config", [("partitioned", "1m_big"), ("replicated", "1m_big"),
                                         ("partitioned", "nstar"), ("replicated", "nstar")])
def test_bench_layouts_world1(mode, config):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--mode", mode, "--config", config, "--steps", "2",
           "--warmup", "1", "--no-secondary", "--no-cpu-baseline", "--no-host-api", "--no-reference-shapes"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["value"] > 0
    assert mode in d["config"]["parallelism"]


def test_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run (no --full) times its steps only, and --dump-outputs writes the last step's
    outputs as float arrays: every member of the include? batch (its first half) answers 1."""
    import numpy as np
    steps, warmup, batch = 3, 1, 1 << 14   # the 10k config's batch
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "10k", "--steps", str(steps),
           "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["ms_per_step"] > 0 and d["value"] > 0
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert key in d, key
    for extra in ("secondary", "multi_gpu_models", "reference_shapes", "cpu_baseline", "host_api", "pmc"):
        assert d[extra] is None, extra
    got = {f: np.load(str(tmp_path / "out" / f)) for f in sorted(os.listdir(str(tmp_path / "out")))}
    assert set(got) == {"include_answers.npy", "any_new.npy", "next_insert_digests.npy", "filter_bytes.npy"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 10**6
    ans = got["include_answers.npy"]
    assert ans.shape == (batch,) and bool((ans[: batch // 2] == 1).all()) and set(np.unique(ans)) <= {0.0, 1.0}
    assert got["any_new.npy"].shape == (steps + warmup,)
    assert got["next_insert_digests.npy"].shape == (batch, 4)
    assert got["filter_bytes.npy"].max() > 0
