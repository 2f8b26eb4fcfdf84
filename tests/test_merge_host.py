"""CPU: the definition of neighbours.mergeSegments (tests/merge_cases.py) gives the answers written out by hand, its
two routes to the contracted table agree on every case, and mergeSegments refuses bad arguments before it touches
the GPU (without a GPU anything that gets past the checks fails as ShepsegHipError instead)."""
import numpy as np
import pytest

import merge_cases as mc
import neighbour_cases as nc


def _tables_equal(got, want):
    return all(np.array_equal(g, w) and g.dtype == w.dtype for (g, w) in zip(got, want))


@pytest.mark.parametrize('four', [True, False])
@pytest.mark.parametrize('keys,answer', [(mc.EXAMPLE_KEYS_A, mc.EXAMPLE_ANSWER_A), (mc.EXAMPLE_KEYS_B, mc.EXAMPLE_ANSWER_B)],
                         ids=['a', 'b'])
def test_example_by_hand(keys, answer, four):
    table = nc.reference_neighbours(nc.EXAMPLE, four)
    assert table[0].tolist() == nc.EXAMPLE_OFFSETS and table[2].tolist() == nc.EXAMPLE_LENGTHS[four]
    size = np.bincount(nc.EXAMPLE.ravel())
    m = mc.reference_merge(table, keys, segSize=size)
    assert m.recode.tolist() == answer['recode'] and m.recode.dtype == np.uint32
    assert m.maxSegId == answer['maxSegId']
    assert m.representative.tolist() == answer['representative']
    assert m.groupSize.tolist() == answer['groupSize']
    assert m.hist.tolist() == answer['hist']
    assert (m.links, m.recordsSorted) == (answer['links'], answer['recordsSorted'])
    assert m.table[0].tolist() == answer['offsets']
    assert m.table[1].tolist() == answer['neighbours']
    assert m.table[2].tolist() == answer['lengths'][four]
    assert mc.reference_merge(table, keys).hist is None


@pytest.mark.parametrize('four', [True, False])
@pytest.mark.parametrize('case', mc.CASES, ids=repr)
def test_graph_route_equals_raster_route(case, four):
    (seg, S, keys, size, table) = mc.build(case, four)
    m = mc.reference_merge(table, keys, case.ignoreKey, case.minBorder, size)
    assert _tables_equal(m.table, mc.raster_route(seg, four, m))
    assert m.recode[0] == 0 and m.recode.max(initial=0) == m.maxSegId
    assert np.array_equal(m.recode[m.representative[1:]], np.arange(1, m.maxSegId + 1))
    assert (np.diff(m.representative[1:].astype(np.int64)) > 0).all()
    assert m.groupSize.sum() == np.count_nonzero(m.recode)
    if size is not None:
        assert np.array_equal(m.hist, np.bincount(m.recode[seg].ravel(), minlength=m.maxSegId + 1))


def test_cases_are_what_they_are_for():
    def merged(name, four=True):
        case = [c for c in mc.CASES if c.name == name][0]
        (seg, S, keys, size, table) = mc.build(case, four)
        return (mc.reference_merge(table, keys, case.ignoreKey, case.minBorder, size), S)

    (m, S) = merged('equal_every_pixel')
    assert m.maxSegId == 1 and m.groupSize.tolist() == [0, 9100]
    (m, S) = merged('equal_enclosed')
    assert m.recode.tolist() == [0, 1, 1, 2]
    (m, S) = merged('equal_half_planes')
    assert m.maxSegId == 1 and len(m.table[1]) == 0
    (m, S) = merged('distinct_random')
    assert np.array_equal(m.recode, np.arange(S + 1)) and m.links == 0
    (m, S) = merged('distinct_sparse_sized')
    assert m.maxSegId == 3 and m.representative.tolist() == nc.SPARSE_IDS.tolist()
    (m, S) = merged('distinct_sparse')
    assert m.maxSegId == nc.SPARSE_MAX
    for name in ('row_descending', 'column_permuted', 'star'):
        (m, S) = merged(name)
        assert m.maxSegId == 1 and m.groupSize[1] == S
    (m, S) = merged('star_top')                 # (its hub took id 1's pixels: id 1 is a group of one without segSize)
    assert m.groupSize.tolist() == [0, 1, S - 1] and m.recode[S] == 2
    (m, S) = merged('star_alternating')
    assert m.groupSize[1] == 1 + (S - 1) // 2 and m.maxSegId == 1 + S // 2
    assert merged('half_planes_300')[0].maxSegId == 1 and merged('half_planes_301')[0].maxSegId == 2
    for four in (True, False):
        (m, S) = merged('through_a_third', four)
        assert m.maxSegId == 1 and m.links == 2          # 1 and 2 are joined, and not by their own border
        assert merged('not_through_a_third', four)[0].maxSegId == 3


# ---- refusals ------------------------------------------------------------------------------------------------------
def _example_table():
    from pyshepseg_amd import neighbours
    (offsets, nbrs, lens) = nc.reference_neighbours(nc.EXAMPLE, True)
    return neighbours.SegmentNeighbours(offsets, nbrs, lens, 3, True)


KEYS = np.array([0, 1, 1, 2], dtype=np.int64)
REFUSALS = [
    ('nb', lambda nb, tmp: dict(nb=(nb.offsets, nb.neighbours, nb.borderLengths))),
    ('key_length', lambda nb, tmp: dict(keyColumn=KEYS[:3])),
    ('key_float', lambda nb, tmp: dict(keyColumn=KEYS.astype(np.float64))),
    ('key_bool', lambda nb, tmp: dict(keyColumn=KEYS.astype(bool))),
    ('key_ndim', lambda nb, tmp: dict(keyColumn=KEYS.reshape(2, 2))),
    ('ignore_float', lambda nb, tmp: dict(ignoreKey=1.0)),
    ('ignore_bool', lambda nb, tmp: dict(ignoreKey=True)),
    ('min_border_zero', lambda nb, tmp: dict(minBorder=0)),
    ('min_border_float', lambda nb, tmp: dict(minBorder=2.0)),
    ('size_length', lambda nb, tmp: dict(segSize=np.ones(5, dtype=np.int64))),
    ('size_float', lambda nb, tmp: dict(segSize=np.ones(4, dtype=np.float32))),
    ('size_negative', lambda nb, tmp: dict(segSize=np.array([1, 3, -2, 3]))),
    ('outfile_without_segfile', lambda nb, tmp: dict(outfile=str(tmp / 'out.npy'))),
    ('npy_without_outfile', lambda nb, tmp: dict(segfile=str(tmp / 'seg.npy'))),
    ('segfile_dtype', lambda nb, tmp: dict(segfile=nc.EXAMPLE.astype(np.int32))),
    ('outfile_not_npy', lambda nb, tmp: dict(segfile=nc.EXAMPLE, outfile=str(tmp / 'out.tif'))),
]


@pytest.mark.parametrize('name,make', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_the_gpu(name, make, tmp_path):
    from pyshepseg_amd import neighbours
    np.save(str(tmp_path / 'seg.npy'), nc.EXAMPLE)
    nb = _example_table()
    kwargs = dict(nb=nb, keyColumn=KEYS)
    kwargs.update(make(nb, tmp_path))
    with pytest.raises(neighbours.PyShepSegNeighboursError):
        neighbours.mergeSegments(**kwargs)


def test_good_arguments_reach_the_gpu():
    """the arguments the refusals are variations of pass the checks: without a GPU the call then fails as every entry
    point does, with one it succeeds"""
    from pyshepseg_amd import _lib, neighbours
    nb = _example_table()
    if _lib.lib().shp_device_count() > 0:
        assert neighbours.mergeSegments(nb, KEYS, ignoreKey=np.int64(5), minBorder=np.uint8(1)).maxSegId == 2
    else:
        with pytest.raises(_lib.ShepsegHipError):
            neighbours.mergeSegments(nb, KEYS, ignoreKey=np.int64(5), minBorder=np.uint8(1))
