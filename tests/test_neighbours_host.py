"""CPU: the numpy definition of the segment-neighbour table on the worked example, the numpy model of the records the
patches hand to the sort (on the figures the GPU cases quote), and the arguments findSegmentNeighbours refuses before
it touches the GPU."""
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


# ---- the model of the patch records (neighbour_cases.patch_records) -------------------------------------------
RECORD_FIGURES = {True: (18000, [4096, 4096, 96, 4096, 4096, 96, 704, 704, 16]),
                  False: (35802, [8160, 8192, 192, 8160, 8192, 192, 1339, 1344, 31])}


@pytest.mark.parametrize('four', [True, False])
def test_patch_records_of_the_constructed_cases(four):
    (per, total) = nc.patch_records(nc.every_pixel_its_own(), four)
    assert total == RECORD_FIGURES[four][0]
    assert nc.patch_record_counts(per).tolist() == RECORD_FIGURES[four][1]
    assert per.dtype == np.int64 and per.shape == (9, 3)
    assert (per[:, 1] == per[:, 2]).all()           # no two lanes side by side hold the same pair
    # one pair everywhere: a record per patch, 9 x 5 patches; in 1-row blocks 257 x 5
    assert nc.patch_records(nc.stripes(), four)[1] == 45
    assert nc.patch_records(nc.stripes(), four, 1)[1] == 1285
    (per, total) = nc.patch_records(nc.stripes(), four, 1)
    assert per.shape == (1285, 3) and (per[:, 0] == 1).all()
    assert nc.patch_records(np.zeros((0, 5), dtype=np.uint32), four)[1] == 0
    assert nc.patch_records(np.zeros((40, 70), dtype=np.uint32), four, 7)[1] == 0


# (n, window pixels, isolated pixels, D, R, records)
TABLE_FILL_FIGURES = {True: [(1023, 490, 1, 1023, 1030, 1023), (1024, 491, 0, 1024, 1029, 1024),
                             (1025, 491, 1, 1025, 1032, 1032)],
                      False: [(1023, 265, 1, 1023, 1175, 1023), (1024, 265, 2, 1024, 1182, 1024),
                              (1025, 265, 3, 1025, 1189, 1189)]}


@pytest.mark.parametrize('four', [True, False])
def test_table_fill_has_exactly_n_distinct_pairs(four):
    for (n, m, isolated, D, R, records) in TABLE_FILL_FIGURES[four]:
        assert nc.table_fill_parts(n, four) == (m, isolated)
        seg = nc.table_fill(n, four)
        assert seg.shape == (96, 192)
        (per, total) = nc.patch_records(seg, four)
        assert per.shape == (9, 3)
        assert per[4].tolist()[:2] == [D, R] and D == n and R != D
        assert not np.delete(per, 4, axis=0).any()          # every pair lies inside patch (1, 1)
        assert total == records == (D if D <= 1024 else R)
        assert per[4, 2] == nc.reference_neighbours(seg, four)[2].sum() // 2


@pytest.mark.parametrize('four', [True, False])
def test_table_wrap_has_one_home_slot(four):
    """1024 distinct pairs with one home slot lie in 1024 slots in a row whatever their order, so the pair that comes
    last is placed by the 1024th probe; and the patch has a run more than pairs, so the route it took shows"""
    chains = nc.table_wrap_chains()
    (a, b) = (chains[:, :-1].ravel(), chains[:, 1:].ravel())
    assert len(np.unique(chains)) == chains.size == 16 * 65 and (a < b).all() and chains.max() < 1 << 21
    assert (nc.pair_home(a, b) == nc.TABLE_WRAP_HOME).all()
    seg = nc.table_wrap()
    assert seg.shape == (96, 192) and seg.dtype == np.uint32
    (per, total) = nc.patch_records(seg, four)
    assert per[4].tolist() == [1024, 1025, 1025]
    assert per[5].tolist() == ([0, 0, 0] if four else [1, 1, 1]) and not np.delete(per, [4, 5], axis=0).any()
    assert total == (1024 if four else 1025)
    # the pairs of patch (1, 1) are the chains' and nothing else
    (offsets, nbrs, lens) = nc.reference_neighbours(seg, four)
    assert len(nbrs) == 2 * total and int(lens.sum()) == 2 * (1025 if four else 1026)


@pytest.mark.parametrize('four', [True, False])
def test_patch_records_of_the_threshold_cases(four):
    z = nc.zone_stripes()
    assert z.shape == (203, 313) and z.dtype == np.uint32
    (offsets, nbrs, lens) = nc.reference_neighbours(z, four)
    assert len(nbrs) == 18 and int(lens.max()) == (12789 if four else 38241)
    assert nc.patch_records(z, four, 1)[1] == (1827 if four else 2635)
    h = nc.hot_segment_top()
    (offsets, nbrs, lens) = nc.reference_neighbours(h, four)
    assert int(h.max()) == 22502 and int(np.diff(offsets)[22502]) == 22500
    assert (nbrs[offsets[22502]:offsets[22503]] < 22502).all()
    assert nc.patch_records(h, four)[1] == (22500 if four else 23100)
    c = nc.calm_then_busy()
    assert c.shape == (96, 128) and c.dtype == np.uint32
    (per, total) = nc.patch_records(c, four, 32)
    assert nc.patch_record_counts(per).tolist() == ([64, 60, 120, 116, 4032, 4000] if four else
                                                    [124, 124, 180, 180, 7969, 7937])
    # the first 32-row block is guessed 32 * 128 / 8 + 1024 = 1536 records: the first two blocks fit, the third
    # needs more than four times that
    counts = nc.patch_record_counts(per)
    assert counts[:4].sum() < 1536 and counts[4:].sum() > 4 * 1536
    w = nc.wide_ids()
    assert int(w.max()) == (1 << 24) + 9 and set(np.unique(w).tolist()) == set(nc.WIDE_IDS.tolist())


@pytest.mark.parametrize('four', [True, False])
def test_patch_records_see_every_pair_once(four):
    """however the raster is cut into blocks and patches"""
    rasters = [nc.EXAMPLE] + [nc.random_labels(shape, top, 7 + shape[0] + top) for shape in nc.OFF_GRID_SHAPES
                              for top in (5, 3000)]
    for seg in rasters:
        want = int(nc.reference_neighbours(seg, four)[2].sum()) // 2
        for rows in (None, 1, 7, 32):
            (per, total) = nc.patch_records(seg, four, rows)
            assert int(per[:, 2].sum()) == want
            assert (per[:, 0] <= per[:, 1]).all() and (per[:, 1] <= per[:, 2]).all()
            assert total <= want
