"""bench.py's --full / --dump-outputs options and the helpers behind --dump-outputs, on CPU tensors (no GPU needed)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_is_not_full_and_dumps_nothing():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_small_output_is_kept_whole_as_float32():
    t = torch.arange(12, dtype=torch.bfloat16).reshape(3, 4)
    s = bench.output_sample(t, n=12)
    assert s.dtype == np.float32 and s.shape == (3, 4) and np.array_equal(s, np.arange(12, dtype=np.float32).reshape(3, 4))


def test_large_output_sample_is_fixed_and_follows_the_values():
    t = torch.arange(10_000, dtype=torch.float32).reshape(10, 1000)
    s1, s2 = bench.output_sample(t, n=500), bench.output_sample(t.clone(), n=500)
    assert s1.dtype == np.float32 and s1.ndim == 1 and 0 < s1.size <= 500
    assert np.array_equal(s1, s2)                          # the same positions in every run
    assert np.all(np.diff(s1) > 0)                         # sorted flat positions, no repeats: here the values are the positions
    tt = t.t().contiguous().t()                            # the same values stored column-major: sampled in logical order
    assert np.array_equal(bench.output_sample(tt, n=500), s1)
    assert not np.array_equal(bench.output_sample(t, n=500, seed=1), s1)


def test_dump_outputs_writes_float_arrays_within_the_limit(tmp_path):
    arrays = {"loss": np.ones(4, np.float32), "loss_sum_count": np.array([4.0, 4.0])}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    for name, a in arrays.items():
        b = np.load(tmp_path / "d" / f"{name}.npy")
        assert b.dtype == a.dtype and np.array_equal(a, b)
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "e"), {"idx": np.arange(3)})
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "f"), {"big": np.zeros(bench.DUMP_LIMIT // 4 + 1, np.float32)})
    assert not (tmp_path / "e").exists() and not (tmp_path / "f").exists()


def test_the_largest_dump_fits_the_limit():
    # loss[B] + the pair + the sample of the gradient / Hessian, at float32
    assert 4 * (256 + bench.DUMP_SAMPLE) + 16 <= bench.DUMP_LIMIT
