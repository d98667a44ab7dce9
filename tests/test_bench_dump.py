"""CPU: what `bench.py --dump-outputs DIR` writes -- y at a fixed sample of rows, the same rows in every run, within the
size a comparison of two builds can hold.  The timed path itself needs a GPU (tests/test_gpu_bench_frontdoor.py)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_samples_fixed_rows_in_float64(tmp_path):
    import bench
    n = 3 * bench.DUMP_ROWS + 17
    y = torch.arange(n, dtype=torch.float64) * 0.5
    for d in ("a", "b"):
        bench.dump_outputs(torch, None, y, 0, n, 1, 0, str(tmp_path / d))
    got = {d: (np.load(tmp_path / d / "y.npy"), np.load(tmp_path / d / "y_rows.npy")) for d in ("a", "b")}
    vals, rows = got["a"]
    assert vals.dtype == np.float64 and rows.dtype == np.float64
    assert np.array_equal(vals, got["b"][0]) and np.array_equal(rows, got["b"][1])      # the same rows in every run
    assert bench.DUMP_ROWS // 2 < len(rows) <= bench.DUMP_ROWS
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n
    assert np.array_equal(vals, rows * 0.5)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20


def test_dump_of_a_small_output_has_every_row(tmp_path):
    """Below the sample size every row is written, in float64 whatever y's type."""
    import bench
    n = 1000
    y = torch.arange(n, dtype=torch.float32) + 1.0
    bench.dump_outputs(torch, None, y, 0, n, 1, 0, str(tmp_path / "all"))
    assert np.array_equal(np.load(tmp_path / "all" / "y_rows.npy"), np.arange(n))
    vals = np.load(tmp_path / "all" / "y.npy")
    assert vals.dtype == np.float64 and np.array_equal(vals, np.arange(n) + 1.0)
