"""CPU: the definition of neighbours.aggregateToGroups (tests/aggregate_cases.py) gives the answers written out by
hand, its three routes agree where all of them are exact, the case raster gives the group sizes it is for, and
aggregateToGroups refuses bad arguments before it touches the GPU (without a GPU anything that gets past the checks
fails as ShepsegHipError instead)."""
import numpy as np
import pytest

import aggregate_cases as ac
import merge_cases as mc
import neighbour_cases as nc
import neighbour_reduce_cases as rc

RECODE = np.array([0, 1, 1, 2], dtype=np.uint32)            # neighbour_cases.EXAMPLE with 1 and 2 merged
COLUMN = np.array([0, 10, 13, 20], dtype=np.float64)
SIZE = np.array([1, 3, 2, 3], dtype=np.int64)               # its histogram


@pytest.mark.parametrize('route', ['exact', 'order', 'fsum'])
def test_example_by_hand(route):
    m = ac.reference_aggregate(RECODE, 2, COLUMN, weights=SIZE, route=route)
    assert m['count'].tolist() == [0, 2, 1] and m['count'].dtype == np.int64
    assert m['weight'].tolist() == [0, 5, 3] and m['weight'].dtype == np.int64
    assert m['min'].tolist() == [-9999, 10, 20] and m['max'].tolist() == [-9999, 13, 20]
    assert m['sum'].tolist() == [-9999, 23, 20] and m['sum'].dtype == np.float64
    assert m['mean'].tolist() == [-9999, 11.5, 20]
    assert m['weightedmean'].tolist() == [-9999, (3 * 10.0 + 2 * 13.0) / 5.0, 20]
    # without weights every weight is 1; an integer column sums as int64
    m = ac.reference_aggregate(RECODE, 2, COLUMN.astype(np.int32), route=route)
    assert m['weight'].tolist() == [0, 2, 1] and m['weightedmean'].tolist() == [-9999, 11.5, 20]
    assert m['sum'].tolist() == [0, 23, 20] and m['sum'].dtype == np.int64
    # holes: 13 ignored, and group 2 emptied; weights that are all 0
    m = ac.reference_aggregate(RECODE, 2, np.array([0, 10, 13, np.nan]), weights=SIZE, ignoreValue=13, missing=7, route=route)
    assert m['count'].tolist() == [0, 1, 0] and m['weight'].tolist() == [0, 3, 0]
    assert m['mean'].tolist() == [7, 10, 7] and m['sum'].tolist() == [7, 10, 7] and m['min'].tolist() == [7, 10, 7]
    m = ac.reference_aggregate(RECODE, 2, COLUMN, weights=np.array([5, 0, 0, 2]), route=route)
    assert m['weightedmean'].tolist() == [-9999, -9999, 20] and m['mean'].tolist() == [-9999, 11.5, 20]
    assert ac.member_csr(RECODE, 2)[0].tolist() == [0, 0, 2, 3] and ac.member_csr(RECODE, 2)[1].tolist() == [1, 2, 3]


def test_int64_sum_wraps_as_numpys():
    big = np.array([0, 2 ** 62, 2 ** 62, 5], dtype=np.int64)
    m = ac.reference_aggregate(RECODE, 2, big)
    assert m['sum'].tolist() == [0, -2 ** 63, 5]


def test_ordered_sum_is_the_stated_order():
    """a plain loop up to LONG; above it the lanes, the butterfly and the chunks -- which differ from the loop on
    real values and agree with every order on integers"""
    x = rc.real_column(9000, 3)
    keep = np.ones(9000, dtype=bool)
    loop = np.float64(0.0)
    for t in x[:rc.LONG]:
        loop = loop + t
    assert ac.ordered_sum(x[:rc.LONG], keep[:rc.LONG]) == loop
    assert ac.ordered_sum(x[:rc.LONG + 1], keep[:rc.LONG + 1]) != loop + x[rc.LONG]
    ints = np.rint(x)
    for n in (rc.LONG + 1, rc.CHUNK, rc.CHUNK + 1, 9000):
        assert ac.ordered_sum(ints[:n], keep[:n]) == ints[:n].sum()
    # one chunk of 65 entries by hand: lane 0 holds x0 + x64, the butterfly adds the 64 lanes pairwise
    acc = x[:64].copy()
    acc[0] = acc[0] + x[64]
    for d in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[np.arange(64) ^ d]
    assert ac.ordered_sum(x[:rc.LONG + 1], keep[:rc.LONG + 1]) != acc[0]        # (257 entries are not these 65)
    y = np.concatenate([x[:65], np.zeros(rc.LONG - 64)])
    assert ac.ordered_sum(y, np.ones(len(y), dtype=bool)) == acc[0]
    half = keep.copy()
    half[::2] = False
    assert ac.ordered_sum(x, half) == ac.ordered_sum(np.where(half, x, 0.0), keep)


def test_case_raster_gives_the_sizes():
    (seg, S, keys, emptyId, base) = ac.raster()
    size = np.bincount(seg.ravel(), minlength=S + 1)
    assert size[emptyId] == 0 and (np.delete(size, [0, emptyId]) == 1).all()
    table = nc.reference_neighbours(seg, True, S)
    assert len(table[1]) <= 100000
    m = mc.reference_merge(table, keys, segSize=size)
    assert m.recode[emptyId] == 0
    assert m.groupSize.tolist() == [0] + ac.RUN_SIZES + [ac.LADDER, ac.LADDER]
    (offsets, members) = ac.member_csr(m.recode, m.maxSegId)
    ladder = members[offsets[-3]:offsets[-2]]
    assert ladder.tolist() == list(range(base, base + 2 * ac.LADDER, 2))        # every other id: interleaved
    assert np.array_equal(np.diff(offsets), m.groupSize)
    for grp in range(1, m.maxSegId + 1):
        ids = members[offsets[grp]:offsets[grp + 1]]
        assert (np.diff(ids.astype(np.int64)) > 0).all() and (m.recode[ids] == grp).all()


# ---- refusals ------------------------------------------------------------------------------------------------------
def _merged():
    from pyshepseg_amd import neighbours
    res = neighbours.MergedSegments()
    (res.recode, res.maxSegId) = (RECODE.copy(), 2)
    return res


ALL = [(s, s) for s in ac.STATS]
REFUSALS = [
    ('merged_tuple', lambda: dict(merged=(RECODE, 2))),
    ('merged_empty', lambda: dict(merged=__import__('pyshepseg_amd.neighbours', fromlist=['x']).MergedSegments())),
    ('merged_is_a_table', lambda: dict(merged=__import__('pyshepseg_amd.neighbours', fromlist=['x']).SegmentNeighbours(
        np.zeros(5, dtype=np.int64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int64), 3, True))),
    ('no_selections', lambda: dict(columnSelections=[])),
    ('column_length', lambda: dict(columnSelections=[(COLUMN[:3], ALL)])),
    ('column_2d', lambda: dict(columnSelections=[(COLUMN.reshape(2, 2), ALL)])),
    ('column_bool', lambda: dict(columnSelections=[(COLUMN > 5, ALL)])),
    ('column_list', lambda: dict(columnSelections=[(COLUMN.tolist(), ALL)])),
    ('unknown_stat', lambda: dict(columnSelections=[(COLUMN, [('m', 'median')])])),
    ('reduce_stat', lambda: dict(columnSelections=[(COLUMN, [('m', 'bordermean')])])),
    ('duplicate_name', lambda: dict(columnSelections=[(COLUMN, [('a', 'min')]), (COLUMN, [('a', 'max')])])),
    ('empty_selection', lambda: dict(columnSelections=[(COLUMN, [])])),
    ('weights_negative', lambda: dict(weights=np.array([1, 3, -2, 3]))),
    ('weights_float', lambda: dict(weights=SIZE.astype(np.float64))),
    ('weights_length', lambda: dict(weights=SIZE[:3])),
    ('weights_2d', lambda: dict(weights=SIZE.reshape(2, 2))),
    ('ignore_text', lambda: dict(ignoreValue='x')),
    ('missing_none', lambda: dict(missingStatsValue=None)),
]


@pytest.mark.parametrize('name,make', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_the_gpu(name, make):
    from pyshepseg_amd import neighbours
    kwargs = dict(merged=_merged(), columnSelections=[(COLUMN, ALL)])
    kwargs.update(make())
    with pytest.raises(neighbours.PyShepSegNeighboursError):
        neighbours.aggregateToGroups(**kwargs)


def test_members_of_refuses_a_group_outside():
    from pyshepseg_amd import neighbours
    for group in (-1, 3):
        with pytest.raises(neighbours.PyShepSegNeighboursError):
            _merged().membersOf(group)


def test_good_arguments_reach_the_gpu():
    """the arguments the refusals are variations of pass the checks: without a GPU the call then fails as every entry
    point does, with one it succeeds -- on a MergedSegments put together by hand, whose recode is uploaded"""
    from pyshepseg_amd import _lib, neighbours
    kwargs = dict(columnSelections=[(COLUMN.astype(np.float32), ALL), (COLUMN.astype(np.int16), [('isum', 'sum')])],
                  weights=SIZE.astype(np.uint8), ignoreValue=np.float32(-1), missingStatsValue=np.int8(7))
    if _lib.lib().shp_device_count() > 0:
        merged = _merged()
        out = neighbours.aggregateToGroups(merged, **kwargs)
        assert out['weightedmean'].tolist() == [7, 11.2, 20] and out['isum'].tolist() == [0, 23, 20]
        assert merged.membersOf(1).tolist() == [1, 2] and merged.memberOffsets.tolist() == [0, 0, 2, 3]
    else:
        with pytest.raises(_lib.ShepsegHipError):
            neighbours.aggregateToGroups(_merged(), **kwargs)
        with pytest.raises(_lib.ShepsegHipError):
            _merged().membersOf(1)
