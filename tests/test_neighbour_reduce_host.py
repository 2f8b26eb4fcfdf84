"""CPU: the numpy model of neighbours.reduceOverNeighbours (tests/neighbour_reduce_cases.py) on the worked example
with numbers written out by hand, the table builder against the rules an uploaded table must keep, and everything
reduceOverNeighbours refuses before it touches the GPU."""
import numpy as np
import pytest

import neighbour_cases as nc
import neighbour_reduce_cases as rc


def example_table():
    (offsets, nbrs, lens) = nc.reference_neighbours(nc.EXAMPLE, True)
    assert offsets.tolist() == [0, 0, 2, 4, 6] and nbrs.tolist() == [2, 3, 1, 3, 1, 2] and lens.tolist() == [1, 2, 1, 2, 2, 2]
    return (offsets, nbrs, lens)


EXAMPLE_COLUMN = [0.0, 10.0, 4.0, 7.0]
# row 1 sees 2 (w 1, v 4) and 3 (w 2, v 7); row 2 sees 1 (1, 10) and 3 (2, 7); row 3 sees 1 (2, 10) and 2 (2, 4), both
# at distance 3 from its own 7: the smaller id is nearest
EXAMPLE_WANT = {'count': [0, 2, 2, 2], 'border': [0, 3, 3, 4], 'min': [-9999, 4, 7, 4], 'max': [-9999, 7, 10, 10],
                'mean': [-9999, 5.5, 8.5, 7], 'bordermean': [-9999, 6, 8, 7], 'meanabsdiff': [-9999, 4, 4, 3],
                'bordertohigher': [0, 0, 3, 2], 'nearest': [0, 3, 3, 1]}
# ignoreValue = 4: segment 2 has no value.  Row 1 keeps 3, row 3 keeps 1; row 2 keeps both but has no own value
EXAMPLE_WANT_IGNORE_4 = {'count': [0, 1, 2, 1], 'border': [0, 2, 3, 2], 'min': [-1, 7, 7, 10], 'max': [-1, 7, 10, 10],
                         'mean': [-1, 7, 8.5, 10], 'bordermean': [-1, 7, 8, 10], 'meanabsdiff': [-1, 3, -1, 3],
                         'bordertohigher': [0, 0, 0, 2], 'nearest': [0, 3, 0, 1]}


def assert_columns(got, want):
    assert sorted(got) == sorted(want)
    for (name, values) in want.items():
        assert got[name].dtype == (np.int64 if name in rc.INT_STATS else np.float64), name
        assert got[name].tolist() == [float(x) if got[name].dtype == np.float64 else x for x in values], name


def test_model_on_the_example():
    (offsets, nbrs, lens) = example_table()
    assert_columns(rc.reference_reduce(offsets, nbrs, lens, np.array(EXAMPLE_COLUMN)), EXAMPLE_WANT)
    for dtype in (np.float32, np.int64):
        assert_columns(rc.reference_reduce(offsets, nbrs, lens, np.array(EXAMPLE_COLUMN, dtype=dtype)), EXAMPLE_WANT)
    assert_columns(rc.reference_reduce(offsets, nbrs, lens, np.array(EXAMPLE_COLUMN), ignoreValue=4, missing=-1),
                   EXAMPLE_WANT_IGNORE_4)
    # NaN is ignored without an ignore value, and a subset of the statistics comes alone
    col = np.array([0.0, 10.0, np.nan, 7.0])
    got = rc.reference_reduce(offsets, nbrs, lens, col, stats=('count', 'nearest', 'meanabsdiff'), missing=-1)
    assert_columns(got, {k: EXAMPLE_WANT_IGNORE_4[k] for k in ('count', 'nearest', 'meanabsdiff')})


def test_model_sums_exactly():
    """terms that cancel: a float64 summation in entry order loses the small one, the model does not"""
    offsets = np.array([0, 0, 3, 3, 3, 3], dtype=np.int64)
    nbrs = np.array([2, 3, 4], dtype=np.uint32)
    lens = np.array([3, 1, 3], dtype=np.int64)
    col = np.array([0.0, 0.0, 1e17, 3.0, -1e17])
    got = rc.reference_reduce(offsets, nbrs, lens, col, withScales=True)
    assert got['mean'][1] == 1.0 and got['bordermean'][1] == 3.0 / 7.0
    assert got['meanabsdiff'][1] == (6e17 + 3.0) / 7.0
    assert got['n'].tolist() == [0, 3, 0, 0, 0] and got['scale:mean'][1] == (2e17 + 3.0) / 3.0
    # a difference that rounds: 1 - 2^-60 is not a float64, the model still adds it exactly
    col = np.array([0.0, 2.0 ** -60, 1.0, 1.0, 1.0])
    got = rc.reference_reduce(offsets, nbrs, np.array([1, 1, 1], dtype=np.int64), col, stats=('meanabsdiff',))
    assert got['meanabsdiff'][1] == 1.0


DEGREE_LISTS = [rc.ISSUE_DEGREES, rc.THRESHOLD_DEGREES, [0], [], [3, 0, 0, 2], [70]]


@pytest.mark.parametrize('degrees', DEGREE_LISTS, ids=lambda d: 'n%d' % len(d))
def test_table_with_degrees_keeps_the_rules(degrees):
    (offsets, nbrs, lens, maxSegId) = rc.table_with_degrees(degrees, 3)
    assert offsets.dtype == np.int64 and nbrs.dtype == np.uint32 and lens.dtype == np.int64
    assert len(offsets) == maxSegId + 2 and maxSegId >= max(degrees, default=0) + (1 if degrees else 0)
    assert np.diff(offsets)[1:1 + len(degrees)].tolist() == list(degrees)
    assert not np.diff(offsets)[1 + len(degrees):].any()
    assert rc.table_violations(offsets, nbrs, lens) == []
    assert len(lens) == 0 or (1 <= int(lens.min()) and int(lens.max()) <= 1 << 17)


def test_span_table_keeps_the_rules():
    deg = rc.span_degrees()
    assert len(deg) == 100000 and deg[49999:50002].tolist() == list(rc.SPAN_LONG_ROWS)
    assert 5.8 < np.delete(deg, [49999, 50000, 50001]).mean() < 6.2
    (offsets, nbrs, lens, maxSegId) = rc.span_table()
    assert maxSegId == 300001 and rc.table_violations(offsets, nbrs, lens) == [] and int(lens.max()) <= 1 << 10
    # the long rows straddle LDS pieces of the rows around them, and chunk edges of their own
    assert int(offsets[50000]) % rc.PIECE != 0 and 300000 % rc.CHUNK != 0


def test_table_violations_names_each_rule():
    (offsets, nbrs, lens) = example_table()

    def broken(which, index, value):
        arrays = [offsets.copy(), nbrs.copy(), lens.copy()]
        arrays[which][index] = value
        return rc.table_violations(*arrays)
    assert broken(0, 1, 1) == ['first'] and broken(0, 3, 1) == ['decreasing']
    assert broken(0, 4, 7) == ['end']
    assert broken(1, 1, 9) == ['range'] and broken(1, 5, 0) == ['range', 'order']
    assert broken(1, 3, 2) == ['self'] and broken(1, 1, 2) == ['order'] and broken(2, 4, 0) == ['length']


def test_argument_errors_need_no_gpu(monkeypatch):
    from pyshepseg_amd import _lib, neighbours

    def no_gpu():
        raise AssertionError('the GPU was asked for')
    monkeypatch.setattr(_lib, 'ctx', no_gpu)
    E = neighbours.PyShepSegNeighboursError
    nb = neighbours.SegmentNeighbours(*example_table(), 3, True)
    col = np.array(EXAMPLE_COLUMN)
    reduce = neighbours.reduceOverNeighbours
    with pytest.raises(E, match='rows'):
        reduce(nb, [(col[:3], [('a', 'mean')])])
    with pytest.raises(E, match='rows'):
        reduce(nb, [(np.zeros(5), [('a', 'mean')])])
    for bad in (col.astype(np.int32), col.astype(np.uint8), col.astype(np.float16), col.astype(np.uint64)):
        with pytest.raises(E, match='dtype'):
            reduce(nb, [(bad, [('a', 'mean')])])
    with pytest.raises(E, match='1-D'):
        reduce(nb, [(col[None], [('a', 'mean')])])
    with pytest.raises(E, match='1-D'):
        reduce(nb, [(EXAMPLE_COLUMN, [('a', 'mean')])])
    with pytest.raises(E, match="unknown statName 'median'"):
        reduce(nb, [(col, [('a', 'mean'), ('b', 'median')])])
    with pytest.raises(E, match="outName 'a' appears twice"):
        reduce(nb, [(col, [('a', 'mean'), ('a', 'min')])])
    with pytest.raises(E, match="outName 'a' appears twice"):
        reduce(nb, [(col, [('a', 'mean')]), (col, [('a', 'min')])])
    with pytest.raises(E, match='empty'):
        reduce(nb, [])
    with pytest.raises(E, match='empty'):
        reduce(nb, [(col, [])])
    with pytest.raises(E, match='empty'):
        reduce(nb, [(col, [('a', 'mean')]), (col, [])])
    for bad in ('x', None, [1], True):
        with pytest.raises(E, match='missingStatsValue must be a number'):
            reduce(nb, [(col, [('a', 'mean')])], missingStatsValue=bad)
    for bad in ('x', [1], False, 1j):
        with pytest.raises(E, match='ignoreValue must be a number'):
            reduce(nb, [(col, [('a', 'mean')])], ignoreValue=bad)
    with pytest.raises(E, match='SegmentNeighbours'):
        reduce(example_table(), [(col, [('a', 'mean')])])
    # a call that passes all of this reaches the GPU
    with pytest.raises(AssertionError, match='the GPU was asked for'):
        reduce(nb, [(col, [('a', 'mean')])], ignoreValue=np.float32(-9999), missingStatsValue=np.int64(-1))


def test_statistic_names_and_types():
    from pyshepseg_amd import neighbours
    assert tuple(sorted(neighbours.REDUCE_STATS)) == tuple(sorted(rc.STATS))
    for (name, (bit, dtype)) in neighbours.REDUCE_STATS.items():
        assert rc.STATS[bit] == name
        assert dtype == (np.int64 if name in rc.INT_STATS else np.float64)
    nb = neighbours.SegmentNeighbours(*example_table(), 3, True)
    assert nb.residentSerial is None and nb.reduceTimings == {}
