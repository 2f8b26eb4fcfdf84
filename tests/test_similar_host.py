"""CPU: the definition of neighbours.mergeSimilarSegments (tests/similar_cases.py) gives the answers written out by
hand, and mergeSimilarSegments refuses bad arguments before it touches the GPU (without a GPU anything that gets past
the checks fails as ShepsegHipError instead)."""
import numpy as np
import pytest

import merge_cases as mc
import neighbour_cases as nc
import similar_cases as sc

# neighbour_cases.EXAMPLE: 1, 2 and 3 all touch.  [0, 10, 13, 20]: d(1,2) = 3, d(2,3) = 7, d(1,3) = 10
COLUMN = np.array([0, 10, 13, 20], dtype=np.float64)
TIE = np.array([0, 10, 13, 16], dtype=np.float64)           # d(2,1) = d(2,3) = 3
# differences (3, 4) between 1 and 2: d = 5 exactly; 3 is far from both
PAIR = [np.array([0, 1, 4, 100], dtype=np.float64), np.array([0, 1, 5, 100], dtype=np.float64)]
HAND = [
    ('at_3', [COLUMN], dict(maxDistance=3), [0, 1, 1, 2]),
    ('chain_7', [COLUMN], dict(maxDistance=7), [0, 1, 1, 1]),
    ('below_3', [COLUMN], dict(maxDistance=2.999), [0, 1, 2, 3]),
    ('mutual', [COLUMN], dict(mutualNearest=True), [0, 1, 1, 2]),
    ('mutual_cut', [COLUMN], dict(mutualNearest=True, maxDistance=2), [0, 1, 2, 3]),
    ('mutual_tie', [TIE], dict(mutualNearest=True), [0, 1, 1, 2]),
    ('pair_at_5', PAIR, dict(maxDistance=5), [0, 1, 1, 2]),
    ('pair_below_5', PAIR, dict(maxDistance=np.nextafter(5.0, 0)), [0, 1, 2, 3]),
]


@pytest.mark.parametrize('four', [True, False])
@pytest.mark.parametrize('name,columns,rule,recode', HAND, ids=[h[0] for h in HAND])
def test_example_by_hand(name, columns, rule, recode, four):
    table = nc.reference_neighbours(nc.EXAMPLE, four)
    assert table[1].tolist() == nc.EXAMPLE_NEIGHBOURS
    m = sc.reference_similar(table, columns, **rule)
    assert m.recode.tolist() == recode and m.recode.dtype == np.uint32
    assert m.maxSegId == max(recode)
    if name == 'mutual':
        assert m.rule.best.tolist() == [0, 2, 1, 2]
    if name == 'mutual_tie':
        assert m.rule.best.tolist() == [0, 2, 1, 2]
    if name == 'at_3':
        # new 1 = {1, 2}, new 2 = {3}: their border is 1-3 plus 2-3
        assert m.representative.tolist() == [0, 1, 3] and m.groupSize.tolist() == [0, 2, 1]
        assert (m.links, m.recordsSorted) == (1, 2)
        assert m.table[2].tolist() == ([4, 4] if four else [8, 8])
    if name == 'pair_at_5':
        (a, b, w) = sc.entries(table)
        assert m.rule.d2[(a == 1) & (b == 2)].tolist() == [25.0] and m.rule.thr2 == 25.0
    if name == 'pair_below_5':
        assert m.rule.thr2 < 25.0


def test_distance_is_symmetric_and_ignores():
    table = nc.reference_neighbours(nc.EXAMPLE, True)
    (a, b, w) = sc.entries(table)
    cols = [np.array([0, 0.1, 0.7, 1e-3]), np.array([0, 1e10, 3.3, -2.5])]
    assert np.array_equal(sc.distance2(cols, a, b), sc.distance2(cols, b, a))
    # an ignored value in one column of two: the id links to nobody, whatever the other column says
    cols = [np.array([0, 1.0, 1.0, 1.0]), np.array([0, 1.0, np.nan, 1.0])]
    assert sc.reference_similar(table, cols, maxDistance=0).recode.tolist() == [0, 1, 2, 1]
    cols = [np.array([0, 1.0, 1.0, 1.0]), np.array([0, 1.0, -1.0, 1.0])]
    assert sc.reference_similar(table, cols, maxDistance=100, ignoreValue=-1).recode.tolist() == [0, 1, 2, 1]
    # an infinite d2 is no candidate even without a threshold
    cols = [np.array([0, 1e200, -1e200, 1e200])]
    m = sc.reference_similar(table, cols, mutualNearest=True)
    assert m.rule.best.tolist() == [0, 3, 0, 1] and m.recode.tolist() == [0, 1, 2, 1]


def test_tail_equals_reference_merge():
    (got, want) = sc.same_as_key_merge()
    for name in ('recode', 'representative', 'groupSize', 'hist'):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert (got.maxSegId, got.links, got.recordsSorted) == (want.maxSegId, want.links, want.recordsSorted)
    assert all(np.array_equal(g, w) for (g, w) in zip(got.table, want.table))


# ---- refusals ------------------------------------------------------------------------------------------------------
def _example_table():
    from pyshepseg_amd import neighbours
    (offsets, nbrs, lens) = nc.reference_neighbours(nc.EXAMPLE, True)
    return neighbours.SegmentNeighbours(offsets, nbrs, lens, 3, True)


REFUSALS = [
    ('nb', lambda nb: dict(nb=(nb.offsets, nb.neighbours, nb.borderLengths))),
    ('no_columns', lambda nb: dict(distanceColumns=[])),
    ('nine_columns', lambda nb: dict(distanceColumns=[COLUMN] * 9)),
    ('columns_not_a_list', lambda nb: dict(distanceColumns=COLUMN)),
    ('column_length', lambda nb: dict(distanceColumns=[COLUMN, COLUMN[:3]])),
    ('column_2d', lambda nb: dict(distanceColumns=[COLUMN.reshape(2, 2)])),
    ('column_bool', lambda nb: dict(distanceColumns=[COLUMN > 5])),
    ('column_complex', lambda nb: dict(distanceColumns=[COLUMN.astype(np.complex128)])),
    ('distance_negative', lambda nb: dict(maxDistance=-1.0)),
    ('distance_nan', lambda nb: dict(maxDistance=float('nan'))),
    ('distance_inf', lambda nb: dict(maxDistance=float('inf'))),
    ('distance_text', lambda nb: dict(maxDistance='3')),
    ('distance_none_without_mutual', lambda nb: dict(maxDistance=None)),
    ('mutual_not_bool', lambda nb: dict(mutualNearest=1)),
    ('ignore_value_text', lambda nb: dict(ignoreValue='x')),
    ('ignore_key_without_keys', lambda nb: dict(ignoreKey=3)),
    ('key_float', lambda nb: dict(keyColumn=COLUMN)),
    ('min_border_zero', lambda nb: dict(minBorder=0)),
    ('size_negative', lambda nb: dict(segSize=np.array([1, 3, -2, 3]))),
    ('segfile_dtype', lambda nb: dict(segfile=nc.EXAMPLE.astype(np.int32))),
]


@pytest.mark.parametrize('name,make', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_the_gpu(name, make):
    from pyshepseg_amd import neighbours
    nb = _example_table()
    kwargs = dict(nb=nb, distanceColumns=[COLUMN], maxDistance=3)
    kwargs.update(make(nb))
    with pytest.raises(neighbours.PyShepSegNeighboursError):
        neighbours.mergeSimilarSegments(**kwargs)


def test_good_arguments_reach_the_gpu():
    """the arguments the refusals are variations of pass the checks: without a GPU the call then fails as every entry
    point does, with one it succeeds"""
    from pyshepseg_amd import _lib, neighbours
    nb = _example_table()
    kwargs = dict(distanceColumns=[COLUMN, COLUMN.astype(np.float32), COLUMN.astype(np.uint8)], maxDistance=np.float32(6),
                  mutualNearest=np.bool_(False), ignoreValue=-1, keyColumn=np.zeros(4, dtype=np.int8), ignoreKey=7,
                  minBorder=np.uint8(1), segSize=np.bincount(nc.EXAMPLE.ravel()))
    if _lib.lib().shp_device_count() > 0:
        # three equal columns: d = 3 sqrt(3) = 5.2 between 1 and 2, above 6 elsewhere
        assert neighbours.mergeSimilarSegments(nb, **kwargs).recode.tolist() == [0, 1, 1, 2]
        assert neighbours.mergeSimilarSegments(nb, [COLUMN], mutualNearest=True).recode.tolist() == [0, 1, 1, 2]
    else:
        with pytest.raises(_lib.ShepsegHipError):
            neighbours.mergeSimilarSegments(nb, **kwargs)
        with pytest.raises(_lib.ShepsegHipError):
            neighbours.mergeSimilarSegments(nb, [COLUMN], mutualNearest=True)
