"""bench.py on the GPU at a small size: a plain run prints the headline line and measures nothing else; --full adds the
measurements that run work of their own (the CPU baseline is left out here: it takes minutes)."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--height", "64", "--width", "96"]
EXTRA = {"allreduce_per_bucket", "roofline", "kernels", "floor_ms", "step_over_floor", "floor_budget", "excess_ms", "forward_only",
         "cpu_baseline"}


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *SMALL, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_measures_only_the_headline():
    d = _bench()
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(d)
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0
    assert not EXTRA & set(d), sorted(EXTRA & set(d))


@pytest.mark.gpu
def test_full_adds_the_other_measurements():
    d = _bench("--full", "--no-cpu-baseline")
    assert {"roofline", "kernels", "floor_ms", "floor_budget", "forward_only"} <= set(d)
    assert "cpu_baseline" not in d and d["ms_per_step"] > 0
