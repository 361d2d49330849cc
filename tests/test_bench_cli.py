"""bench.py's options and its output dump, on the host: a plain run is the headline measurement only (--full adds the
rest), and --dump-outputs writes float32 arrays within its size budget, cut to the same seeded sample on every run."""
import os

import numpy as np
import pytest

import bench


def test_plain_run_is_the_default_and_steps_are_checked():
    a = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 5 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_write_outputs_keeps_small_sets_whole(tmp_path):
    arrays = {"sr_output": np.linspace(-1, 1, 24, dtype=np.float32).reshape(2, 3, 2, 2),
              "loss": np.array(0.25, dtype=np.float32), "parameters": np.arange(7, dtype=np.float64)}
    bench.write_outputs(arrays, str(tmp_path / "d"))
    got = _read(str(tmp_path / "d"))
    assert sorted(got) == sorted(arrays)
    for k, a in arrays.items():
        assert got[k].dtype == np.float32 and got[k].shape == a.shape
        assert np.array_equal(got[k], a.astype(np.float32))


def test_write_outputs_samples_large_sets_reproducibly(tmp_path):
    arrays = {"big": np.arange(3000, dtype=np.float32).reshape(30, 100), "small": np.arange(400, dtype=np.float32) + 1e4,
              "loss": np.array(3.0, dtype=np.float32)}
    budget = 2000
    for d in ("a", "b"):
        bench.write_outputs(arrays, str(tmp_path / d), budget=budget)
    a, b = _read(str(tmp_path / "a")), _read(str(tmp_path / "b"))
    assert sorted(a) == sorted(arrays)
    assert sum(v.nbytes for v in a.values()) <= budget
    for k in arrays:
        assert np.array_equal(a[k], b[k]), "the sample of %s differs between two runs" % k
        assert a[k].dtype == np.float32
    assert a["loss"].item() == 3.0
    for k in ("big", "small"):
        flat = arrays[k].reshape(-1)
        assert 0 < a[k].size < flat.size and a[k].ndim == 1
        assert np.all(np.diff(a[k]) > 0) and np.all(np.isin(a[k], flat)), "a sample is a subset in index order"
    # every array keeps the same fraction of its elements
    assert abs(a["big"].size / 3000.0 - a["small"].size / 400.0) < 0.01
