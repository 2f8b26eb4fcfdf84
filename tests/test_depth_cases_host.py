"""CPU: the model of tests/depth_cases.py against the literal definition of depth2, what the cases of
tests/test_gpu_depths.py reach, and everything depths.calcSegmentDepths refuses or derives on the host."""
import os
import re

import numpy as np
import pytest

import depth_cases as dc
from conftest import ROOT


# ---- the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(36))
def test_model_is_the_definition(seed):
    """1 to 4 labels and label 0 in up to 5 x 5 cells, blown up by 1 to 3"""
    seg = dc.blown_up(seed)
    assert max(seg.shape) <= 15
    assert np.array_equal(dc.reference_depth2(seg), dc.brute_depth2(seg))


def test_blown_up_rasters_cover_their_ranges():
    rasters = [dc.blown_up(seed) for seed in range(36)]
    assert {int(r.max()) for r in rasters} >= {1, 2, 3, 4} and any((r == 0).any() for r in rasters)
    values = set()
    for r in rasters:
        values |= set(np.unique(dc.reference_depth2(r)).tolist())
    # label 0, edge pixels, a diagonal neighbour, depth 2 straight and past a corner, depth 3
    assert values >= {0, 1, 2, 4, 5, 9}


@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (9, 1), (2, 2), (7, 12), (12, 7), (2 * dc.HALO + 3, 11)], ids=str)
def test_model_one_label_closed_form(shape):
    (h, w) = shape
    (y, x) = np.mgrid[0:h, 0:w]
    want = np.minimum(np.minimum(y + 1, h - y), np.minimum(x + 1, w - x)) ** 2
    assert np.array_equal(dc.reference_depth2(dc.one_label(h, w)), want)
    assert np.array_equal(dc.rectangle_depth2(h, w), want)


def test_model_stripes_closed_form():
    """the closed form that stands in for the model on the thin rasters, on small ones"""
    for (h, w, along) in ((9, 50, False), (50, 9, True), (3, 40, False), (40, 3, True)):
        assert np.array_equal(dc.reference_depth2(dc.stripes(h, w, 3, along)), dc.stripes_depth2(h, w, 3, along))
        assert sorted(np.unique(dc.stripes(h, w, 3, along)).tolist()) == [1, 2, 3]


def test_model_columns_worked_example():
    """a 4 x 5 rectangle of label 2 beside a column of label 1, label 0 below: written out by hand"""
    seg = dc.u32([[1, 2, 2, 2, 2, 2],
                  [1, 2, 2, 2, 2, 2],
                  [1, 2, 2, 2, 2, 2],
                  [1, 2, 2, 2, 2, 2],
                  [0, 0, 0, 0, 0, 0]])
    (cols, d2) = dc.reference_depths(seg, (('c0', 0), ('c1', 1), ('c15', 1.5)), origin=(10, 100), maxSegId=3)
    assert d2.tolist() == [[1, 1, 1, 1, 1, 1], [1, 1, 4, 4, 4, 1], [1, 1, 4, 4, 4, 1], [1, 1, 1, 1, 1, 1], [0] * 6]
    assert cols['maxDepth2'].tolist() == [0, 1, 4, 0] and cols['sumDepth2'].tolist() == [0, 4, 14 + 24, 0]
    assert cols['interiorRow'].tolist() == [0, 10, 11, 0] and cols['interiorCol'].tolist() == [0, 100, 102, 0]
    assert cols['c0'].tolist() == [0, 4, 20, 0] and cols['c1'].tolist() == [0, 0, 6, 0] and cols['c15'].tolist() == [0, 0, 6, 0]
    assert cols['maxDepth'].tolist() == [-9999.0, 1.0, 2.0, -9999.0]
    assert cols['meanDepth2'].tolist() == [-9999.0, 1.0, 1.9, -9999.0]
    assert cols['depthRatio'].tolist() == [-9999.0, np.pi / 4, np.pi * 4 / 20, -9999.0]


# ---- the constants ----------------------------------------------------------------------------------------------------
def test_constants_are_the_headers():
    with open(os.path.join(ROOT, 'pyshepseg_amd', 'csrc', 'segdepth.h')) as f:
        text = f.read()
    for (mine, theirs) in dc.HEADER_NAMES.items():
        m = re.search(r'^#define\s+%s\s+(\d+)u?\b' % theirs, text, flags=re.M)
        assert m, theirs
        assert int(m.group(1)) == getattr(dc, mine), theirs
    from pyshepseg_amd import depths
    assert depths.MAX_CORE_AREAS == dc.CORES and len(dc.EIGHT_CORES) == dc.CORES


# ---- what the cases reach ---------------------------------------------------------------------------------------------
def test_geometry_straddles_every_size():
    heights = {h for (h, _w) in dc.GEOMETRY}
    widths = {w for (_h, w) in dc.GEOMETRY}
    for n in (dc.TH, dc.BAND, dc.PH, 2 * dc.BAND):
        assert {n - 1, n, n + 1} <= heights, n
    for n in (dc.HALO, dc.TW, 2 * dc.TW):
        assert {n - 1, n, n + 1} <= widths, n
    assert {(1, 1), (2, 2)} <= set(dc.GEOMETRY) and 1 in heights and 1 in widths
    rasters = dc.geometry_rasters((dc.BAND + 1, dc.TW + 1))
    assert any((r == 0).any() for r in rasters) and any(not (r == 0).any() for r in rasters)
    deepest = [int(dc.reference_depth2(r).max()) for r in rasters]
    assert min(deepest) <= 2 and max(deepest) >= 100    # single pixels, and segments ten pixels deep


def test_one_label_squares_sit_on_both_sides_of_the_halo():
    for odd in (True, False):
        for (depth, deferred) in ((dc.HALO - 1, False), (dc.HALO, False), (dc.HALO + 1, True)):
            seg = dc.square_of_depth(depth, odd)
            d2 = dc.rectangle_depth2(*seg.shape)
            assert d2.max() == depth * depth and (d2 == d2.max()).sum() == (1 if odd else 4)
            assert dc.window_deferred(seg).any() == deferred, (depth, odd)
    big = dc.square_of_depth(4 * dc.HALO, False)
    assert dc.window_deferred(big).sum() > 1000


def test_shapes_reach_what_they_are_named_for():
    for name in dc.SHAPES_DEFERRED:
        assert dc.window_deferred(dc.shape(name)).any(), name
    for name in dc.SHAPES_NOT_DEFERRED:
        assert not dc.window_deferred(dc.shape(name)).any(), name
    # radii round the halo, in label 0 and in another label
    for (name, inside) in (('disc_in_0_below_halo', 0), ('disc_in_0_at_halo', 0), ('disc_in_2_above_halo', 2), ('ring_in_0', 0),
                           ('ring_in_2', 2)):
        seg = dc.shape(name)
        assert sorted(np.unique(seg).tolist()) == sorted({1, inside}), name
    # a nearest foreign pixel that lies diagonally: depth2 is a sum of two squares, neither of them 0, somewhere in
    # the shape, and not reached along the row or the column
    for name in ('ell', 'u_shape', 'comb'):
        seg = dc.shape(name)
        d2 = dc.reference_depth2(seg).astype(np.int64)
        g = dc.column_distance(seg)
        rowwise = np.zeros_like(g)
        for y in range(seg.shape[0]):
            (first, last) = dc._row_runs(seg[y])
            x = np.arange(seg.shape[1])
            rowwise[y] = np.minimum(x - first + 1, last + 1 - x)
        assert ((seg != 0) & (d2 < np.minimum(g, rowwise) ** 2)).any(), name
    # two parts of equal depth: the first part's pixel
    (cols, d2) = dc.reference_depths(dc.shape('two_parts'))
    deepest = np.argwhere(d2 == d2.max())
    assert len(deepest) == 2 and cols['interiorRow'][5] == deepest[0][0] and cols['interiorCol'][5] == deepest[0][1]
    # the one-pixel hole and slit are felt
    seg = dc.shape('pinhole')
    assert dc.reference_depth2(seg).max() < dc.rectangle_depth2(*seg.shape).max()


def test_table_cases_sit_on_both_sides_of_the_slots():
    own = dc.every_pixel_its_own()
    assert own.shape[0] > dc.PH and own.shape[1] > dc.TW and len(np.unique(own[:dc.PH, :dc.TW])) > dc.SLOTS
    for n in (dc.SLOTS - 1, dc.SLOTS, dc.SLOTS + 1):
        seg = dc.labels_in_patch(n)
        assert seg.shape == (dc.PH, dc.TW) and len(np.unique(seg)) == n and seg.min() == 1
    sparse = dc.sparse_high_ids()
    ids = np.unique(sparse)
    assert ids[0] == 0 and len(ids) <= 6 and np.diff(ids).min() > 30000


# ---- the host checks of the call --------------------------------------------------------------------------------------
def test_core_area_depths_become_integers():
    from pyshepseg_amd import depths
    assert depths.depth2q(0) == 0 and depths.depth2q(1) == 1 and depths.depth2q(1.5) == 2 and depths.depth2q(2) == 4
    assert depths.depth2q(32768) == 2 ** 30 and depths.depth2q(np.float32(2.5)) == 6 and depths.depth2q(8 ** 0.5) in (7, 8)
    assert depths.depth2q(8 ** 0.5) == int(np.floor(8 ** 0.5 * 8 ** 0.5))
    for bad in (-0.5, 32768.5, float('nan'), float('inf'), True, None, 'deep', 1j):
        with pytest.raises(depths.PyShepSegDepthsError, match='edge depth'):
            depths.depth2q(bad)
    assert depths.checkCoreAreas([('a', 0), ('b', 1.5)]) == [('a', 0), ('b', 2)]
    assert depths.checkCoreAreas(()) == []


def test_refusals_come_before_the_gpu(monkeypatch):
    from pyshepseg_amd import _lib, depths

    def no_gpu():
        raise AssertionError('the GPU was asked for')
    monkeypatch.setattr(_lib, 'ctx', no_gpu)
    seg = dc.one_label(3, 3)
    E = depths.PyShepSegDepthsError
    nine = [('c%d' % k, k) for k in range(9)]
    for (kw, text) in (({'coreAreas': nine}, '9 core areas'),
                       ({'coreAreas': [('a', 1), ('a', 2)]}, 'named twice'),
                       ({'coreAreas': [('maxDepth2', 1)]}, 'fixed column'),
                       ({'coreAreas': [('depthRatio', 1)]}, 'fixed column'),
                       ({'coreAreas': [('a', -1)]}, 'edge depth'),
                       ({'coreAreas': [('a', 32769)]}, 'edge depth'),
                       ({'coreAreas': [('a', float('nan'))]}, 'edge depth'),
                       ({'coreAreas': [('a', True)]}, 'edge depth'),
                       ({'coreAreas': [('a', 'x')]}, 'edge depth'),
                       ({'coreAreas': [('a',)]}, 'pairs'),
                       ({'coreAreas': 5}, 'pairs'),
                       ({'path': 'window'}, 'path'),
                       ({'path': None}, 'path'),
                       ({'origin': (-1, 0)}, 'origin'),
                       ({'maxSegId': -2}, 'maxSegId')):
        with pytest.raises(E, match=text):
            depths.calcSegmentDepths(seg, **kw)
    with pytest.raises(E):
        depths.calcSegmentDepths(np.zeros((3, 3), dtype=np.float32))
    with pytest.raises(AssertionError, match='GPU was asked'):
        depths.calcSegmentDepths(seg, coreAreas=[('c%d' % k, k) for k in range(8)], path='envelope')


def test_derived_columns_from_a_table_written_out_by_hand():
    """depthColumnsFromTable on rows written by hand: the key's halves, the origin, the missing value, the divisions"""
    from pyshepseg_amd import depths
    ncols = 7

    def key(d2, y, x):
        return (d2 << 32) | (0xFFFFFFFF - (y * ncols + x))
    table = np.zeros((4, 11), dtype=np.uint64)
    table[1, :5] = [12, 30, key(9, 2, 3), 12, 5]
    table[3, :5] = [1, 1, key(1, 0, 6), 1, 0]
    cols = depths.depthColumnsFromTable(table, ncols, (100, 1000), [('all', 0), ('inner', 2)], -1.5)
    assert sorted(cols) == sorted(depths.COUNT_COLUMNS + depths.DERIVED_COLUMNS + ('all', 'inner'))
    assert cols['maxDepth2'].tolist() == [0, 9, 0, 1] and cols['sumDepth2'].tolist() == [0, 30, 0, 1]
    assert cols['interiorRow'].tolist() == [0, 102, 0, 100] and cols['interiorCol'].tolist() == [0, 1003, 0, 1006]
    assert cols['all'].tolist() == [0, 12, 0, 1] and cols['inner'].tolist() == [0, 5, 0, 0]
    assert cols['maxDepth'].tolist() == [-1.5, 3.0, -1.5, 1.0]
    assert cols['meanDepth2'].tolist() == [-1.5, 2.5, -1.5, 1.0]
    assert cols['depthRatio'].tolist() == [-1.5, np.pi * 9 / 12, -1.5, np.pi]
    for k in depths.COUNT_COLUMNS + ('all', 'inner'):
        assert cols[k].dtype == np.int64
    for k in depths.DERIVED_COLUMNS:
        assert cols[k].dtype == np.float64
