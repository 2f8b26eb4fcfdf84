"""CPU: the numpy model of the distributed shape table's split (shapes_dist_helpers) against the definition, the reach
conditions of the cases the GPU test runs, and the refusals of calcSegmentShapesDistributed that need no device."""
import types

import numpy as np
import pytest

import shape_cases as SC
import shapes_dist_helpers as SD


@pytest.mark.parametrize('name,seg,S,cuts', SD.hostCases(), ids=[c[0] for c in SD.hostCases()])
def test_the_ranks_tables_add_up_to_the_reference(name, seg, S, cuts):
    """counts and sums add modulo 2^64, extents combine by min / max over the ranks that hold the id"""
    tables = [SD.rankTable(seg, cuts[r], cuts[r + 1], S) for r in range(len(cuts) - 1)]
    (counts, sums) = SD.combine(tables)
    (wantC, wantS) = SC.reference_shapes(seg, S)
    for k in SC.COUNTS:
        assert counts[k].dtype == np.int64 and np.array_equal(counts[k], wantC[k]), (name, k)
    for k in SC.SUMS:
        assert sums[k].dtype == np.uint64 and np.array_equal(sums[k], wantS[k]), (name, k)
    # two ranks' sums past 2^63 each: the model adds them modulo 2^64, as the table's 64-bit adds do
    a = np.array([0, (1 << 63) + 5], dtype=np.uint64)
    one = ({k: np.array([0, 1], dtype=np.int64) for k in SC.COUNTS}, {k: a.copy() for k in SC.SUMS})
    assert all(v.tolist() == [0, 10] for v in SD.combine([one, one])[1].values())


@pytest.mark.parametrize('name', SD.GPU_CASES)
def test_the_cases_reach_what_they_are_meant_for(name):
    from pyshepseg_amd import dist_shapes
    assert dist_shapes.SHAPE_RECORD_BYTES == 96
    (seg, S, cuts) = SD.caseByName(name)
    m = SD.model(seg, cuts, S)
    SD.assertReach(name, seg, cuts, S, m)
    tables = [SD.rankTable(seg, cuts[r], cuts[r + 1], S) for r in range(len(cuts) - 1)]
    assert np.array_equal(m['areas'], np.stack([t[0]['area'] for t in tables]))
    # the exchange's account of itself
    assert sum(m['picked']) == sum(m['records']) and sum(m['folded']) == m['straddlers']
    live = sum(1 for r in range(len(cuts) - 1) if cuts[r + 1] > cuts[r])
    assert m['exchange_bytes'] == 96 * sum(m['records']) + 8 * seg.shape[1] * live
    assert all(i['exchange_bytes'] == m['exchange_bytes'] for i in m['info'])


def test_world_one_exchanges_nothing():
    (seg, S, _cuts) = SD.caseByName('A-w2-four')
    m = SD.model(seg, [0, seg.shape[0]], S)
    assert (m['exchange_bytes'], m['records'], m['halo_rows'], m['straddlers']) == (0, [0], 0, 0)


def test_an_engine_without_the_device_path_is_refused():
    from pyshepseg_amd import distributed, dist_shapes, shapes
    assert distributed.calcSegmentShapesDistributed is dist_shapes.calcSegmentShapesDistributed
    assert distributed.deviceShapes is dist_shapes.deviceShapes
    dres = types.SimpleNamespace(maxSegId=3, hist=np.zeros(4, dtype=np.int64))
    with pytest.raises(shapes.PyShepSegShapesError, match='device engine'):
        distributed.calcSegmentShapesDistributed(types.SimpleNamespace(c=None), None, dres)


def test_a_merge_without_histogram_is_refused():
    from pyshepseg_amd import distributed, neighbours, shapes
    m = neighbours.MergedSegmentsShare()
    (m.maxSegId, m.rowRange) = (3, (0, 4))
    assert m.hist is None
    eng = types.SimpleNamespace(c=None, nCols=5, shapesOnDevice=None)
    with pytest.raises(shapes.PyShepSegShapesError, match='no histogram'):
        distributed.calcSegmentShapesDistributed(eng, None, m)
    # with a histogram the rows are asked for next
    m.rowRange = None
    with pytest.raises(shapes.PyShepSegShapesError, match='no recoded rows'):
        distributed.calcSegmentShapesDistributed(eng, types.SimpleNamespace(onDevice=True), m, hist=np.zeros(4, dtype=np.int64))


def test_the_table_tail_is_shared_with_the_one_gpu_function():
    """columnsFromTable: the packed extent words split, the float columns from shapeColumnsFromSums"""
    from pyshepseg_amd import shapes
    table = np.zeros((2, 11), dtype=np.uint64)
    table[1] = [4, 2, 6, 2, 10, 3, 8, 8, 4, (1 << 32) | 0, (2 << 32) | 1]       # a 2 x 2 square at (0, 1)
    (columns, sums) = shapes.columnsFromTable(table, -1)
    assert list(columns) == list(shapes.COUNT_COLUMNS + shapes.DERIVED_COLUMNS) and list(sums) == list(shapes.SUM_COLUMNS)
    assert [int(columns[k][1]) for k in shapes.COUNT_COLUMNS] == [4, 0, 1, 1, 2, 8, 8, 4]
    assert columns['centroidRow'].tolist() == [-1.0, 0.5] and columns['centroidCol'].tolist() == [-1.0, 1.5]
    assert columns['bboxFill'][1] == 1.0 and sums['sumRowCol'].tolist() == [0, 3]
