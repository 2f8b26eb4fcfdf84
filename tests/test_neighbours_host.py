"""CPU: the numpy definition of the segment-neighbour table on the worked example, and the arguments
findSegmentNeighbours refuses before it touches the GPU."""
import numpy as np
import pytest

import neighbour_cases as nc


@pytest.mark.parametrize('four', [True, False])
def test_definition_on_the_example(four):
    (offsets, nbrs, lens) = nc.reference_neighbours(nc.EXAMPLE, four)
    assert offsets.dtype == np.int64 and nbrs.dtype == np.uint32 and lens.dtype == np.int64
    assert offsets.tolist() == nc.EXAMPLE_OFFSETS
    assert nbrs.tolist() == nc.EXAMPLE_NEIGHBOURS
    assert lens.tolist() == nc.EXAMPLE_LENGTHS[four]


def test_definition_on_the_constructed_cases():
    """the figures the GPU cases quote"""
    (offsets, nbrs, lens) = nc.reference_neighbours(nc.every_pixel_its_own(), False)
    assert len(nbrs) == 71604 and int(np.diff(offsets).max()) == 8
    for (four, want) in ((True, [300, 300]), (False, [898, 898])):
        (offsets, nbrs, lens) = nc.reference_neighbours(nc.half_planes(), four)
        assert offsets.tolist() == [0, 0, 1, 2] and nbrs.tolist() == [2, 1] and lens.tolist() == want
    (offsets, nbrs, lens) = nc.reference_neighbours(nc.hot_segment(), True)
    assert int(np.diff(offsets).max()) == 150 * 150 == int(np.diff(offsets)[1])
    (offsets, nbrs, lens) = nc.reference_neighbours(nc.sparse_ids(), True, nc.SPARSE_MAX)
    assert len(offsets) == nc.SPARSE_MAX + 2
    assert set(np.flatnonzero(np.diff(offsets)).tolist()) == {5, 70000, 1 << 20}
    (offsets, nbrs, lens) = nc.reference_neighbours(nc.enclosed_by_zeros(), False)
    assert np.diff(offsets).tolist() == [0, 1, 1, 0]


def test_columns_and_rows_of_a_table():
    from pyshepseg_amd import neighbours
    (offsets, nbrs, lens) = nc.reference_neighbours(nc.EXAMPLE, False)
    t = neighbours.SegmentNeighbours(offsets, nbrs, lens, 3, False)
    cols = t.columns
    assert cols['numNeighbours'].tolist() == [0, 2, 2, 2] and cols['numNeighbours'].dtype == np.int64
    assert cols['borderLength'].tolist() == [0, 6, 6, 8] and cols['borderLength'].dtype == np.int64
    (ids, ln) = t.neighboursOf(3)
    assert ids.tolist() == [1, 2] and ln.tolist() == [4, 4] and ids.base is nbrs
    assert len(t.neighboursOf(0)[0]) == 0
    with pytest.raises(neighbours.PyShepSegNeighboursError):
        t.neighboursOf(4)


def test_argument_errors_need_no_gpu(monkeypatch):
    from pyshepseg_amd import _lib, neighbours

    def no_gpu():
        raise AssertionError('the GPU was asked for')
    monkeypatch.setattr(_lib, 'ctx', no_gpu)
    E = neighbours.PyShepSegNeighboursError
    with pytest.raises(E, match='2-D uint32'):
        neighbours.findSegmentNeighbours(nc.EXAMPLE.astype(np.int32))
    with pytest.raises(E, match='2-D uint32'):
        neighbours.findSegmentNeighbours(nc.EXAMPLE.astype(np.uint64))
    with pytest.raises(E, match='2-D uint32'):
        neighbours.findSegmentNeighbours(nc.EXAMPLE.ravel())
    with pytest.raises(E, match='2-D uint32'):
        neighbours.findSegmentNeighbours(nc.EXAMPLE[None])
    with pytest.raises(E, match='2-D uint32'):
        neighbours.findSegmentNeighbours('labels.tif')
    with pytest.raises(E, match='maxSegId'):
        neighbours.findSegmentNeighbours(nc.EXAMPLE, maxSegId=-1)
    with pytest.raises(E, match='maxSegId'):
        neighbours.findSegmentNeighbours(nc.EXAMPLE, maxSegId=2.5)
    with pytest.raises(E, match='too large'):
        neighbours.findSegmentNeighbours(nc.EXAMPLE, maxSegId=0xFFFFFFFF)
