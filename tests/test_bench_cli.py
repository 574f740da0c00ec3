"""bench.py's command line and its --dump-outputs writer.  CPU only (no step runs here)."""
import os
import sys

import numpy as np

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert a.full is False and a.dump_outputs is None


def test_full_and_dump_options(monkeypatch, tmp_path):
    a = _parse(monkeypatch, "--full", "--no-config4", "--no-cpu-baseline", "--dump-outputs", str(tmp_path))
    assert a.full is True and a.no_config4 and a.no_cpu_baseline and a.dump_outputs == str(tmp_path)


def test_write_outputs_small_arrays_whole(tmp_path):
    rng = np.random.default_rng(0)
    arrays = {"a": rng.random((5, 3)), "b": rng.random(7).astype(np.float32)}
    shapes = bench.write_outputs(str(tmp_path / "d"), arrays)
    assert shapes == {"a": [5, 3], "b": [7]}
    for k, v in arrays.items():
        got = np.load(tmp_path / "d" / (k + ".npy"))
        assert got.dtype == v.dtype and np.array_equal(got, v)


def test_write_outputs_files_are_finite(tmp_path):
    """Non-finite entries are written as 0 with their kind beside them (1 NaN, 2 +inf, 3 -inf); a later run into the
    same directory without any leaves no stale side file."""
    a = np.array([[1.0, np.nan], [np.inf, -np.inf], [0.0, -2.0]])
    d = tmp_path / "d"
    shapes = bench.write_outputs(str(d), {"a": a, "b": np.ones(3, dtype=np.float32)})
    assert shapes == {"a_nonfinite": [3, 2], "a": [3, 2], "b": [3]}
    got, code = np.load(d / "a.npy"), np.load(d / "a_nonfinite.npy")
    assert got.dtype == code.dtype == np.float64
    assert np.array_equal(got, [[1.0, 0.0], [0.0, 0.0], [0.0, -2.0]])
    assert np.array_equal(code, [[0, 1], [2, 3], [0, 0]])
    assert not (d / "b_nonfinite.npy").exists()
    bench.write_outputs(str(d), {"a": np.zeros((3, 2)), "b": np.ones(3, dtype=np.float32)})
    assert not (d / "a_nonfinite.npy").exists()


def test_write_outputs_caps_with_a_fixed_sample(tmp_path, monkeypatch):
    """An array over its share of the byte budget is cut to the same rows, in row order, on every call; the files
    together stay within the budget."""
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    big = np.arange(1000 * 4, dtype=np.float64).reshape(1000, 4)  # 32 000 B > 1024 B share
    small = np.arange(10, dtype=np.float32)
    s1 = bench.write_outputs(str(tmp_path / "x"), {"big": big, "small": small})
    s2 = bench.write_outputs(str(tmp_path / "y"), {"big": big, "small": small})
    assert s1 == s2 == {"big": [32, 4], "small": [10]}
    x, y = np.load(tmp_path / "x" / "big.npy"), np.load(tmp_path / "y" / "big.npy")
    assert np.array_equal(x, y)
    rows = (x[:, 0] // 4).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(x, big[rows])
    assert np.array_equal(np.load(tmp_path / "x" / "small.npy"), small)
    assert sum(np.load(os.path.join(tmp_path, "x", f)).nbytes for f in os.listdir(tmp_path / "x")) <= 4096
