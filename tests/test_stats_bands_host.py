"""CPU: the combined fast selection of calcPerSegmentStatsTiledBands (tilingstats.makeBandStatsSelection) is
makeFastStatsSelection of the bands' selections one after the other, and its name checks raise before
anything is read."""
import numpy as np
import pytest


def _flat(bandSelections):
    return [sel for (_b, s) in bandSelections for sel in s]


@pytest.mark.parametrize('bandSelections', [
    [(1, [('b1_mean', 'mean'), ('b1_min', 'min'), ('b1_p30', 'percentile', 30)]),
     (3, [('b3_n', 'pixcount'), ('b3_sd', 'stddev')])],
    [(2, [('a', 'stddev'), ('b', 'median')]),
     (1, [('c', 'pixcount')]),
     (2, [('d', 'percentile', 95), ('e', 'mean'), ('f', 'mode'), ('g', 'max')])],
])
def test_band_selection_is_the_concatenation(bandSelections):
    from pyshepseg_amd import tilingstats as ts
    (fast, bandOfStat, nInt, nFloat) = ts.makeBandStatsSelection(bandSelections)
    flat = _flat(bandSelections)
    (want, wInt, wFloat) = ts.makeFastStatsSelection(list(range(len(flat))), flat)
    assert fast.dtype == ts.STATSSELFAST_DTYPE and np.array_equal(fast, want)
    assert (nInt, nFloat) == (wInt, wFloat)
    assert list(bandOfStat) == [k for (k, (_b, s)) in enumerate(bandSelections) for _ in s]
    # the global column index runs through all entries, the per-type index through the entries' columns of that type
    assert list(fast[:, ts.STATSEL_GLOBALCOLINDEX]) == list(range(len(flat)))
    for t in (ts.STAT_DTYPE_INT, ts.STAT_DTYPE_FLOAT):
        idx = fast[fast[:, ts.STATSEL_COLTYPE] == t, ts.STATSEL_COLARRAYINDEX]
        assert list(idx) == list(range(len(idx)))
    pc = [i for (i, s) in enumerate(flat) if s[1] == 'percentile']
    assert [int(fast[i, ts.STATSEL_PARAM]) for i in pc] == [flat[i][2] for i in pc]
    assert all(int(fast[i, ts.STATSEL_PARAM]) == ts.NOPARAM for i in range(len(flat)) if i not in pc)


def test_band_selection_errors():
    from pyshepseg_amd import tilingstats as ts
    with pytest.raises(ts.PyShepSegStatsError):
        ts.makeBandStatsSelection([])
    with pytest.raises(ts.PyShepSegStatsError, match='selects no statistic'):
        ts.makeBandStatsSelection([(1, [('a', 'mean')]), (2, [])])
    with pytest.raises(ts.PyShepSegStatsError, match='more than once'):
        ts.makeBandStatsSelection([(1, [('a', 'mean')]), (2, [('b', 'min'), ('a', 'max')])])
    with pytest.raises(ts.PyShepSegStatsError, match='more than once'):
        ts.makeBandStatsSelection([(1, [('a', 'mean'), ('a', 'min')])])
    with pytest.raises(ts.PyShepSegStatsError, match='Unknown statistic'):
        ts.makeBandStatsSelection([(1, [('a', 'average')])])


def test_name_checks_come_before_any_read():
    """a file that does not exist is never opened when the selection is refused"""
    from pyshepseg_amd import tilingstats as ts
    with pytest.raises(ts.PyShepSegStatsError, match='more than once'):
        ts.calcPerSegmentStatsTiledBands('no_such_image.npy', [(1, [('a', 'mean')]), (2, [('a', 'min')])],
                                         'no_such_labels.npy')
    with pytest.raises(ts.PyShepSegStatsError):
        ts.calcPerSegmentStatsTiledBands('no_such_image.npy', [], 'no_such_labels.npy')
