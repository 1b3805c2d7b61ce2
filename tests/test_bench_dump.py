"""bench.py --dump-outputs on CPU: the file format, the 64 MB bound and the fixed sample of a large output; --steps is checked."""
import os
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_writes_float_arrays_within_the_budget(tmp_path):
    sys.path.insert(0, REPO)
    import bench
    big = torch.arange(3_000_000, dtype=torch.float32)
    arrays = {"loss_terms": [0.5, 0.25, float("nan")], "depth": torch.ones(2, 1, 4, 6, dtype=torch.bfloat16),
              "params": big, "acc": torch.arange(5, dtype=torch.float64)}
    budget = 4 << 20
    info = bench.dump_outputs(str(tmp_path / "a"), arrays, budget=budget)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["acc.npy", "depth.npy", "loss_terms.npy", "params.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget
    lt = np.load(tmp_path / "a" / "loss_terms.npy")
    assert lt.dtype == np.float64 and lt[:2].tolist() == [0.5, 0.25] and np.isnan(lt[2])
    d = np.load(tmp_path / "a" / "depth.npy")
    assert d.dtype == np.float32 and d.shape == (2, 1, 4, 6) and (d == 1).all()
    assert np.load(tmp_path / "a" / "acc.npy").dtype == np.float64
    p = np.load(tmp_path / "a" / "params.npy")
    assert p.dtype == np.float32 and 0 < p.size < big.numel() and info["params"] == ((3_000_000,), p.size)
    assert (np.diff(p) > 0).all()                  # a sorted sample of distinct elements
    bench.dump_outputs(str(tmp_path / "b"), arrays, budget=budget)
    assert np.array_equal(p, np.load(tmp_path / "b" / "params.npy"))      # the same sample on every run


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0", "--stub"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
