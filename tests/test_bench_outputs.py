"""bench.py's plain run (no ``--full``) and ``--dump-outputs`` on the CPU path with a tiny model: the
result line keeps the headline keys and leaves out what ``--full`` adds, and two runs with the same
arguments write the same arrays."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Two plain runs with identical arguments -> [(result line, {name: array})] (run once, shared)."""
    base = tmp_path_factory.mktemp("bench")
    out = []
    for name in ("a", "b"):
        d = base / name
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
               "--cpu", "--model", "vit_tiny_patch16", "--batch-per-gpu", "4", "--image-size", "64",
               "--dump-outputs", str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(base),
                           env=dict(os.environ, OMP_NUM_THREADS="2"))
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        out.append((json.loads(lines[0]), {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}))
    return out


def test_plain_run_result_line(runs):
    for res, _ in runs:
        assert res["metric"].startswith("pretrain images/sec") and res["unit"] == "images/sec"
        assert res["higher_is_better"] is True and res["dtype"] == "fp32"  # --cpu: the fp32 path
        assert res["steps"] == 2 and res["warmup"] == 1
        assert res["ms_per_step"] > 0
        # images/sec and ms_per_step describe the same timed steps (the line rounds the value to 0.01)
        assert res["value"] == pytest.approx(res["config"]["global_batch"] * 1000.0 / res["ms_per_step"], abs=0.01)
        for k in ("weight_checksum", "replica_weight_checksum_spread", "collective_sweep", "dp_ready_spans"):
            assert k not in res  # --full only


def test_dump_outputs_are_reproducible(runs):
    (res, a), (_, b) = runs
    assert set(a) == set(b) == {"metric_loss", "metric_learning_rate", "master_weights", "grad"}
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), (k, a[k].dtype)
        assert np.array_equal(a[k], b[k]), k  # same seeded inputs, same seeded sample indices
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["master_weights"].shape == a["grad"].shape == (4 << 20,)  # larger buffers: the fixed sample
    assert np.isfinite(a["grad"]).all() and np.count_nonzero(a["grad"]) > 0
    assert float(a["metric_loss"].reshape(-1)[0]) == pytest.approx(res["config"]["final_loss"], abs=1e-5)
