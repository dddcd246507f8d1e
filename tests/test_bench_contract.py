"""bench.py driver-contract smoke: the JSON line must parse and carry
the agreed fields (the round driver consumes it verbatim)."""

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--cpu",
         "--nodes", "300", "--jobs", "150", "--pods-per-job", "4",
         "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    j = json.loads(line)
    for field in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                  "ms_per_step", "higher_is_better", "scaling",
                  "vs_baseline", "dtype", "data", "config"):
        assert field in j, f"missing {field}"
    assert j["metric"] == "pods_scheduled_per_sec"
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1
    assert j["higher_is_better"] is True
    assert j["data"] == "synthetic"
    assert j["value"] > 0 and j["vs_baseline"] > 0
    assert "WARNING" not in out.stdout      # all pods bound every step


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last step's placements as float64 .npy;
    the same arguments give the same arrays run after run; --full is
    accepted and keeps the result line."""
    import numpy as np
    dumps = []
    for run, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / run
        out = subprocess.run(
            [sys.executable, os.path.join(ROOT, "bench.py"), "--cpu",
             "--nodes", "100", "--jobs", "30", "--pods-per-job", "4", "--mix",
             "--steps", "1", "--warmup", "0", "--dump-outputs", str(d)]
            + extra,
            capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
        j = json.loads(line)
        assert j["steps"] == 1 and j["ms_per_step"] > 0
        assert sorted(p.name for p in d.iterdir()) == \
            ["node_pod_count.npy", "pod_node.npy"]
        dumps.append({p.stem: np.load(p) for p in d.iterdir()})
        pod_node = dumps[-1]["pod_node"]
        counts = dumps[-1]["node_pod_count"]
        assert pod_node.dtype == np.float64 and counts.dtype == np.float64
        assert pod_node.shape == (j["config"]["global_batch"],)
        assert counts.shape == (100,)
        assert pod_node.min() >= 0 and pod_node.max() < 100  # all bound
        assert counts.sum() == pod_node.size
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name
