"""CPU: the sampling and the file format of `bench.py --dump-outputs` (the arrays two builds are compared by)."""
import os

import numpy as np
import pytest

import bench


def test_dump_sample_is_fixed_sorted_and_distinct():
    a = bench.dump_sample(40000, 1536, bench.DUMP_SEED)
    assert np.array_equal(a, bench.dump_sample(40000, 1536, bench.DUMP_SEED))
    assert len(a) == 1536 and a[0] >= 0 and a[-1] < 40000
    assert (np.diff(a) > 0).all()
    assert not np.array_equal(a, bench.dump_sample(40000, 1536, bench.DUMP_SEED + 1))


def test_dump_sample_keeps_small_ranges_whole():
    assert np.array_equal(bench.dump_sample(700, 1536, bench.DUMP_SEED), np.arange(700))


def test_write_outputs(tmp_path):
    arrays = {'x': np.arange(5, dtype=np.float64), 'y': np.ones((2, 3), dtype=np.float32)}
    bench.write_outputs(str(tmp_path / 'out'), arrays)
    assert sorted(os.listdir(tmp_path / 'out')) == ['x.npy', 'y.npy']
    for (name, a) in arrays.items():
        got = np.load(tmp_path / 'out' / (name + '.npy'))
        assert got.dtype == a.dtype and np.array_equal(got, a)


def test_write_outputs_refuses_other_dtypes_and_oversize(tmp_path):
    with pytest.raises(AssertionError):
        bench.write_outputs(str(tmp_path), {'x': np.arange(5, dtype=np.uint32)})
    with pytest.raises(AssertionError):
        bench.write_outputs(str(tmp_path), {'x': np.zeros(bench.DUMP_MAX_BYTES // 8 + 1)})
