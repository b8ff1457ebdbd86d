"""bench.py's plain run: warmup, the timed steps and the result line only, and --dump-outputs writing
the last timed step's verdicts -- equal to the semantic oracle's over the same batches."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_the_last_steps_verdicts(engine, oracle_built, tmp_path):
    steps, warmup, txns, history = 3, 2, 400, 20000
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
           str(warmup), "--txns", str(txns), "--history", str(history), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == steps and out["warmup"] == warmup and out["full"] is False
    assert out["value"] > 0 and out["unit"] == "txns/s" and out["higher_is_better"] is True
    assert abs(out["value"] - txns / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    # nothing but the timed region was measured or checked
    for k in ("parity", "cpu_baseline", "sync", "device_bound", "roofline", "phase_ms_per_batch",
              "h2d_inclusive_txns_per_s", "total_txns_per_s", "roofline_pass_txns_per_s"):
        assert out[k] is None, k
    assert out["kernels"] == {}
    assert os.listdir(tmp_path / "out") == ["verdicts.npy"]
    got = np.load(tmp_path / "out" / "verdicts.npy")
    assert got.dtype == np.float32 and got.shape == (txns,)

    # the same batches through the oracle: the timed batches are added before the region starts, so
    # their TooOld tests see the oldest version the warmup left (add_oldest)
    sys.path.insert(0, ROOT)
    import bench

    args = SimpleNamespace(workload="c2", txns=txns, history=history, too_old_frac=0.0, seed=1)
    p = bench.workload_params(args)
    kb, ko, vers = bench.shard_history(args, p, args.seed, 0, 1, 10_000_000)
    ref = oracle_built.OracleConflictSet()
    ref.load_history(kb, ko, vers)
    batches = bench.make_batches(args, p, warmup + steps, 1, 10_000_000)
    for i, (pb, now, new_oldest) in enumerate(batches):
        if i in (0, warmup):  # each pass packs all its batches before its first detect
            packed_at = ref.oldest_version
        want, _ = ref.detect(pb, now, new_oldest, add_oldest=packed_at)
    np.testing.assert_array_equal(got, want.astype(np.float32))
