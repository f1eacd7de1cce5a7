"""bench.py on the GPU at a small size: a plain run prints the headline fields only and writes the timed steps' outputs;
--full adds the roofline / host / kernel figures and writes the same outputs for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config")
FULL_ONLY = ("roofline", "roofline_classes", "roofline_step", "host_enqueue_ms", "cpu_baseline", "kernels", "kernel_timing",
             "kernel_source_hash")


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8",
           "--hw", "64", "--dump-outputs", str(out_dir)] + list(extra)
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_and_full_lines_and_dumped_outputs(tmp_path):
    plain = _bench(tmp_path / "plain")
    for k in HEADLINE:
        assert k in plain, k
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["ms_per_step"] > 0 and plain["dtype"] == "bf16"
    assert abs(plain["value"] - 8 * 1e3 / plain["ms_per_step"]) <= 2e-3 * plain["value"]
    assert not any(k in plain for k in FULL_ONLY), [k for k in FULL_ONLY if k in plain]

    full = _bench(tmp_path / "full", "--full", "--no-cpu-baseline")
    for k in HEADLINE + FULL_ONLY:
        assert k in full, k
    assert full["roofline"]["kernel"] in full["roofline_classes"]

    files = sorted(os.listdir(tmp_path / "plain"))
    assert files == sorted(os.listdir(tmp_path / "full"))
    assert "stats.loss.npy" in files and "model.fc.weight.npy" in files
    total = 0
    for f in files:
        a = np.load(tmp_path / "plain" / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        total += a.nbytes
        # the same seeded inputs, the same (bit-identical) steps: the same outputs
        assert np.array_equal(a, np.load(tmp_path / "full" / f)), f
    assert total <= 64 << 20
