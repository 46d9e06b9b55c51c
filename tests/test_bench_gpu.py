"""bench.py on the GPU: a plain run prints the headline and what the timed steps themselves recorded, nothing that takes runs of its
own; --full adds those after the timed region."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("ms_per_step_untapped", "mma_core", "cpu_baseline", "cpu_baseline_c2_est", "secondary")


def _bench_line(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2"] + args,
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_only():
    out = _bench_line([])
    assert out["unit"] == "tokens/s" and out["higher_is_better"] is True and out["dtype"] == "bf16" and out["steps"] == 2
    assert abs(out["value"] - 2 * 655 / (out["ms_per_step"] / 1e3)) / out["value"] < 1e-3
    assert out["roofline"]["bound"] == "mfma" and 0.0 < out["roofline"]["frac"] < 1.0 and "mma_kernel" in out
    assert [k for k in FULL_ONLY if k in out] == []


def test_full_run_adds_the_untapped_loop_and_the_attention_core():
    out = _bench_line(["--full", "--no-cpu-baseline"])
    assert out["ms_per_step_untapped"] > 0.0 and out["mma_core"]["avg_launch_ms"] > 0.0
    # --no-cpu-baseline; the secondary legs run at the headline's batch of 8 only
    assert "cpu_baseline" not in out and "secondary" not in out
