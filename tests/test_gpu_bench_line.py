"""`python bench.py` at N=1: a plain run prints the headline line and nothing it does not need; `--full` adds the measurements
that take runs of their own (HBM calibration, fp64 leg, CPU baseline, box clocks) after the timed steps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDARY = ("cpu_baseline", "f64", "two_folds", "northstar", "c5", "fm_c4", "rank", "box")


def _line(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--workload", "small"] + list(extra)
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_and_full_bench_lines():
    plain = _line()
    assert plain["metric"] == "SGD rating-updates/sec, CAMF_CI k=128" and plain["unit"] == "rating-updates/s"
    assert plain["higher_is_better"] is True and plain["dtype"] == "f32" and plain["steps"] == 2 and plain["warmup"] == 1
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["roofline"]["bound"] == "hbm" and plain["roofline"]["frac"] > 0
    assert not any(key in plain for key in SECONDARY), sorted(plain)
    assert "peak_measured" not in plain["roofline"] and "secondary" not in plain["config"]

    full = _line("--full")
    assert full["metric"] == plain["metric"] and full["unit"] == plain["unit"] and full["dtype"] == plain["dtype"]
    assert full["value"] > 0 and full["ms_per_step"] > 0
    assert full["config"]["final_loss"] == pytest.approx(plain["config"]["final_loss"], rel=1e-6)     # the same seeded epochs
    assert "copy_GBps" in full["roofline"]["peak_measured"]
    assert full["f64"]["value"] > 0 and full["f64"]["dtype"] == "f64"
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["five_fold"]["cores"] == 5
    assert isinstance(full["box"], dict) and "f64" in full["config"]["secondary"]
