"""GPU: bench.py's own contract on the tiny workload -- a plain run times exactly --steps steps and adds nothing else to
its line, --dump-outputs writes the same arrays from run to run (same arguments, same inputs), and --full still runs
the HIP-event profiled pass."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", *args],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_and_dump_outputs_repeat(tmp_path):
    runs = [_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for line in runs:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["roofline"] is None and "parity" not in line and "cpu_baseline" not in line
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"loss.npy", "recon.npy", "latent.npy", "state.quantize_t.embed.npy"} <= set(names)
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b), n
    assert float(np.load(tmp_path / "a" / "loss.npy")) == pytest.approx(runs[0]["final_loss"], abs=1e-6)


def test_full_run_profiled_pass():
    line = _bench("--steps", "4", "--warmup", "1", "--full", "--no-cpu-baseline", "--prof-all")
    assert line["steps"] == 4 and line["ms_per_step"] > 0
    assert line["kernel_ms_per_step"] and line["algorithmic_gflop_per_step"] > 0
