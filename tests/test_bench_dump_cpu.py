"""bench.py --dump-outputs writer (dump_outputs): float64 stays, everything else becomes float32, and
arrays beyond the byte budget are cut to a fixed sample that is the same on every call.  CPU only."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import REPO


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_dump_mod", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_budget_is_below_64_mb(bench):
    assert bench.DUMP_BUDGET <= 64 * 10 ** 6 - 4096


def test_small_arrays_are_written_whole(bench, tmp_path):
    a = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    b = torch.arange(6, dtype=torch.uint8).reshape(2, 3)
    bench.dump_outputs(str(tmp_path / "d"), {"a": a, "b": b, "c": np.float32([1.5])})
    assert sorted(os.listdir(tmp_path / "d")) == ["a.npy", "b.npy", "c.npy"]
    ra, rb = np.load(tmp_path / "d" / "a.npy"), np.load(tmp_path / "d" / "b.npy")
    assert ra.dtype == np.float64 and np.array_equal(ra, a.numpy())
    assert rb.dtype == np.float32 and np.array_equal(rb, b.numpy().astype(np.float32))


def test_large_arrays_are_sampled_at_fixed_indices(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4096)
    big = np.arange(5000, dtype=np.float32).reshape(50, 100)      # 20000 B > its 2048-B share
    small = np.arange(10, dtype=np.float64)
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    one, two = np.load(tmp_path / "one" / "big.npy"), np.load(tmp_path / "two" / "big.npy")
    assert one.shape == (512,) and one.dtype == np.float32 and np.array_equal(one, two)
    assert np.all(np.diff(one) > 0) and np.array_equal(one, big.reshape(-1)[one.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "one" / "small.npy"), small)
    total = sum(os.path.getsize(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one"))
    assert total <= 4096 + 2 * 128                                  # payload within the budget (+ .npy headers)
