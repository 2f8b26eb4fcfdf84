"""GPU: shapes.calcSegmentShapes against the numpy definition (tests/shape_cases.py), numpy.array_equal on every
counted column and every sum: everything is integer, nothing has a tolerance.  The derived float columns must be
bit for bit shapeColumnsFromSums of the model's counts and sums, the same host function.

The kernel (csrc/segshape.h) sums the runs of 32 x 64 patches in an LDS table keyed by label, so the shapes are chosen
by where that can go wrong: pixels and sides on patch edges, corners and the raster's rim; runs of length 1 and of a
whole wavefront, runs that end on lane 63 and begin on lane 0; a patch with 2048 labels, one label in every patch.

T = 512 (SHAPE_SLOTS, shape_cases.TABLE_SLOTS) is the table's slot count: a patch with more than T distinct labels
takes the overflow route, every run straight to the device table.  Cases: exactly T - 1, T and T + 1 distinct labels
in one patch, and T labels that share one home slot (the last probe of the trip round the table).

Not covered: labels of 2^31 and more in a successful table (88 bytes per id: 189 GB)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import neighbour_cases as nc
import shape_cases as sc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

T = sc.TABLE_SLOTS


def calc(seg, **kw):
    from pyshepseg_amd import shapes
    return shapes.calcSegmentShapes(seg, **kw)


def assert_shapes(got, want, origin=(0, 0), missing=-9999):
    """want: (counts, sums) of the model"""
    from pyshepseg_amd import shapes
    (counts, sums) = want
    n = len(counts['area'])
    assert got.maxSegId == n - 1 and got.origin == tuple(origin)
    assert sorted(got.columns) == sorted(shapes.COUNT_COLUMNS + shapes.DERIVED_COLUMNS)
    assert sorted(got.sums) == sorted(shapes.SUM_COLUMNS)
    for k in sc.COUNTS:
        assert got.columns[k].dtype == np.int64 and np.array_equal(got.columns[k], counts[k]), k
    for k in sc.SUMS:
        assert got.sums[k].dtype == np.uint64 and np.array_equal(got.sums[k], sums[k]), k
    derived = shapes.shapeColumnsFromSums(counts, sums, missing)
    for k in shapes.DERIVED_COLUMNS:
        assert got.columns[k].dtype == np.float64 and got.columns[k].tobytes() == derived[k].tobytes(), k
    empty = counts['area'] == 0
    for k in shapes.DERIVED_COLUMNS:
        assert np.all(got.columns[k][empty] == missing), k


def check(seg, maxSegId=None, origin=(0, 0), chunkPixels=None, model=sc.reference_shapes):
    got = calc(seg, maxSegId=maxSegId, origin=origin, chunkPixels=chunkPixels)
    assert_shapes(got, model(seg, maxSegId, origin), origin)
    return got


@functools.lru_cache(maxsize=None)
def real_raster(name):
    if name == 'mosaic':
        with np.load(os.path.join(GOLDEN, 'ci_scenario_1000.npz')) as z:
            seg = z['mosaic']
    elif name == 'random1024':
        seg = nc.random_labels((1024, 1024), 39999, 1)
    else:
        with np.load(os.path.join(GOLDEN, 'tile_synth128_null.npz')) as z:
            seg = z[name]
    seg = np.ascontiguousarray(seg, dtype=np.uint32)
    seg.setflags(write=False)
    return seg


@functools.lru_cache(maxsize=None)
def real_reference(name):
    return sc.reference_shapes(real_raster(name))


# ---- the worked example -----------------------------------------------------------------------------------------------
def test_example():
    got = calc(sc.EXAMPLE)
    assert got.maxSegId == 3
    for (k, v) in sc.EXAMPLE_COUNTS.items():
        assert got.columns[k].tolist() == v, k
    for (k, v) in sc.EXAMPLE_SUMS.items():
        assert got.sums[k].tolist() == v, k
    assert got.columns['centroidRow'][1:].tolist() == [1 / 3, 0.5, 1 + 2 / 3]
    assert got.columns['bboxFill'][1:].tolist() == [0.75, 1.0, 0.75]
    assert got.columns['centroidRow'][0] == -9999 and got.deviceMs > 0 and got.timings['total'] > 0
    # in another place, with another missing value
    moved = calc(sc.EXAMPLE, origin=(10, 1000), missingStatsValue=-1.5)
    assert moved.columns['rowMin'].tolist() == [0, 10, 10, 11] and moved.columns['colMax'].tolist() == [0, 1001, 1002, 1002]
    assert_shapes(moved, sc.reference_shapes(sc.EXAMPLE, None, (10, 1000)), (10, 1000), -1.5)


# ---- shapes off the patch grid ------------------------------------------------------------------------------------
@pytest.mark.parametrize('top', [5, 3000])
@pytest.mark.parametrize('shape', sc.OFF_GRID_SHAPES, ids=lambda s: '%dx%d' % s)
def test_shapes_off_the_patch_grid(shape, top):
    check(nc.random_labels(shape, top, 7 + shape[0] + top))


def test_empty_rasters():
    for shape in ((0, 5), (5, 0)):
        got = calc(np.zeros(shape, dtype=np.uint32), maxSegId=2)
        assert got.columns['area'].tolist() == [0, 0, 0] and got.columns['elongation'].tolist() == [-9999.0] * 3
    assert calc(np.zeros((3, 3), dtype=np.uint32)).maxSegId == 0


# ---- run aggregation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [sc.stripes, sc.half_planes, sc.runs_end_on_lane_63], ids=lambda f: f.__name__)
def test_runs(case):
    """runs of length 1; full 64-lane runs and a segment in every patch of its half; runs that end on lane 63 and
    begin on lane 0"""
    check(case())


# ---- table population ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [sc.every_pixel_its_own, sc.hot_segment], ids=lambda f: f.__name__)
def test_table_population(case):
    """2048 distinct labels per full patch (the overflow route); one label in every patch among thousands of
    one-pixel segments"""
    check(case())


@pytest.mark.parametrize('distinct', [T - 1, T, T + 1])
def test_table_fill(distinct):
    """T fills every slot, T + 1 is the first to overflow"""
    seg = sc.table_fill(distinct)
    patch = seg[sc.PATCH_ROWS:2 * sc.PATCH_ROWS, sc.PATCH_COLS:2 * sc.PATCH_COLS]
    assert len(np.unique(patch)) == distinct
    check(seg)


def test_table_wrap():
    seg = sc.table_wrap()
    labels = np.unique(seg)[1:]
    assert len(labels) == T and np.all(sc.label_home(labels) == sc.TABLE_WRAP_HOME)
    check(seg)


# ---- ids ----------------------------------------------------------------------------------------------------------
def test_sparse_ids():
    got = check(sc.sparse_ids(), maxSegId=sc.SPARSE_MAX)
    assert np.count_nonzero(got.columns['area']) == 3
    assert not got.columns['rowMin'][1:5].any() and not got.sums['sumRowRow'][1:5].any()


def test_labels_past_2_24():
    check(sc.wide_ids(), maxSegId=sc.WIDE_MAX)


def test_enclosed_by_zeros():
    got = check(sc.enclosed_by_zeros())
    assert got.columns['outerBorder'][3] == got.columns['perimeter'][3] == 60
    assert got.columns['perimeter'][1] - got.columns['outerBorder'][1] == 10


def test_label_above_max_seg_id():
    from pyshepseg_amd import shapes
    seg = np.array(real_raster('seg_final'))
    top = int(seg.max())
    with pytest.raises(shapes.PyShepSegShapesError, match='segment id %d is above maxSegId %d' % (top, top - 1)):
        calc(seg, maxSegId=top - 1)
    # the largest of several, wherever it lies
    seg[5:9, 5:9] = top + 7
    seg[127, 127] = 0xFFFFFFF0
    seg[64, 0] = top + 100
    with pytest.raises(shapes.PyShepSegShapesError, match='segment id %d is above maxSegId %d' % (0xFFFFFFF0, top)):
        calc(seg, maxSegId=top, chunkPixels=7 * 128)
    # in an area of one label only
    solid = np.full((40, 70), 9, dtype=np.uint32)
    with pytest.raises(shapes.PyShepSegShapesError, match='segment id 9 is above maxSegId 8'):
        calc(solid, maxSegId=8)
    check(solid, maxSegId=9)


# ---- wide coordinates ---------------------------------------------------------------------------------------------
def test_tall_and_wide():
    """r^2 and c^2 pass 2^32"""
    for seg in sc.tall_and_wide():
        got = check(seg)
        assert int(max(got.sums['sumRowRow'].max(), got.sums['sumColCol'].max())) > 2 ** 44


def test_every_sum_wraps():
    seg = nc.random_labels((40, 70), 9, 3)
    origin = (2 ** 32 - 40, 2 ** 32 - 70)
    got = check(seg, origin=origin, model=sc.reference_shapes_pyint)
    assert got.columns['rowMax'].max() == 2 ** 32 - 1 and got.columns['colMax'].max() == 2 ** 32 - 1
    here = check(seg, model=sc.reference_shapes_pyint)
    for k in ('bboxFill', 'compactness', 'elongation', 'orientation'):
        assert got.columns[k].tobytes() == here.columns[k].tobytes(), k


# ---- blocks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [1, 31, 32, 33])
@pytest.mark.parametrize('name', ['mosaic', 'seg_final', 'random1024'])
def test_block_independence(name, rows):
    """random1024 in blocks of 31 rows ends in a block of one row"""
    seg = real_raster(name)
    if (name, rows) == ('random1024', 31):
        assert seg.shape[0] % rows == 1
    assert_shapes(calc(seg, chunkPixels=rows * seg.shape[1]), real_reference(name))


@pytest.mark.parametrize('name', ['mosaic', 'seg_final', 'random1024'])
def test_one_block(name):
    assert_shapes(calc(real_raster(name)), real_reference(name))


# ---- sources ------------------------------------------------------------------------------------------------------
def test_npy_path_and_result_object(tmp_path):
    from pyshepseg_amd import tiling
    seg = real_raster('mosaic')
    path = str(tmp_path / 'labels.npy')
    np.save(path, seg)
    want = real_reference('mosaic')
    assert_shapes(calc(path), want)
    assert_shapes(calc(path, chunkPixels=33 * seg.shape[1], maxSegId=int(seg.max())), want)
    res = tiling.TiledSegmentationResult()
    res.segimg = seg
    res.maxSegId = int(seg.max()) + 2               # the result's own maxSegId is taken
    got = calc(res, chunkPixels=7 * seg.shape[1])
    assert_shapes(got, sc.reference_shapes(seg, int(seg.max()) + 2))


@pytest.mark.parametrize('zeros', [False, True], ids=['no label 0', 'with label 0'])
def test_merged_array(zeros):
    """``area`` is the merge's ``hist``.  Row 0 of ``hist`` counts the pixels of label 0, which is no segment here
    (row 0 of every shape column is 0): the whole column is compared on the mosaic with its zeros made label 1, and
    on the mosaic as it is the rows from 1, with ``hist[0]`` the zeros of the raster."""
    from pyshepseg_amd import neighbours
    seg = real_raster('mosaic')
    assert (seg == 0).any()
    if not zeros:
        seg = np.maximum(seg, 1)
    S = int(seg.max())
    keys = (np.arange(S + 1) % 3).astype(np.int64)
    nb = neighbours.findSegmentNeighbours(seg, True, maxSegId=S)
    m = neighbours.mergeSegments(nb, keys, segfile=seg)
    assert m.outDev is None and 0 < m.maxSegId < S
    s = calc(m)
    assert_shapes(s, sc.reference_shapes(m.segimg, m.maxSegId))
    if zeros:
        assert s.columns['area'][0] == 0 and m.hist[0] == (seg == 0).sum()
        assert np.array_equal(s.columns['area'][1:], m.hist[1:])
    else:
        assert np.array_equal(s.columns['area'], m.hist)


def test_device_resident_labels_and_their_merge():
    """labels kept in HBM by the tiled segmentation, read in place, whole and in row blocks; the recoded raster a merge
    leaves in HBM"""
    from pyshepseg_amd import _lib, tiling, neighbours
    (nrows, ncols) = (300, 902)
    ras = tiling.DeviceRaster.synth(3, 3, nrows, ncols)
    try:
        cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=3)
        rd = tiling.doTiledShepherdSegmentation(ras, tiling._KEEP_ON_DEVICE, tileSize=256, overlapSize=64,
                                                minSegmentSize=30, numClusters=12, fixedKMeansInit=True,
                                                concurrencyCfg=cfg)
        m = None
        try:
            c = _lib.ctx()

            def download(outDev):
                img = np.empty((nrows, ncols), dtype=np.uint32)
                c.check(c._L.shp_dev_download(c.handle, img.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(outDev[0]),
                                              img.nbytes))
                return img
            S = rd.maxSegId
            got = {rows: calc(rd, chunkPixels=None if rows is None else ncols * rows) for rows in (None, 1, 33)}
            got['given'] = calc(rd, maxSegId=S)
            rd_max = rd.maxSegId
            rd.maxSegId = None                      # the largest label is then found on the device
            got['reduced'] = calc(rd)
            rd.maxSegId = rd_max
            segimg = download(rd.outDev)
            nb = neighbours.findSegmentNeighbours(rd, True, maxSegId=S)
            keys = (np.arange(S + 1) % 3).astype(np.int64)
            m = neighbours.mergeSegments(nb, keys, segfile=rd)
            assert m.segimg is None and m.outDev is not None
            merged = calc(m)
            mergedimg = download(m.outDev)
            mhist = m.hist
            M = m.maxSegId
        finally:
            if m is not None:
                tiling.freeDeviceOutput(m)
            tiling.freeDeviceOutput(rd)
    finally:
        ras.free()
    assert int(segimg.max()) == S
    want = sc.reference_shapes(segimg)
    for key in got:
        assert_shapes(got[key], want)
    assert_shapes(calc(segimg), want)
    assert_shapes(merged, sc.reference_shapes(mergedimg, M))
    # (row 0 of the histogram counts the raster's zeros, which are no segment: test_merged_array)
    assert merged.columns['area'][0] == 0 and mhist[0] == (mergedimg == 0).sum()
    assert np.array_equal(merged.columns['area'][1:], mhist[1:])


# ---- identities on the GPU's own outputs ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['mosaic', 'seg_final'])
def test_perimeter_identity(name):
    from pyshepseg_amd import neighbours
    seg = real_raster(name)
    s = calc(seg)
    nb = neighbours.findSegmentNeighbours(seg, fourConnected=True)
    assert np.array_equal(s.columns['perimeter'], nb.columns['borderLength'] + s.columns['outerBorder'])


def test_edge_pixels_equal_the_spatial_statistic():
    """userFuncNumEdgePixels (four-connected) over a band of ones without null pixels"""
    from pyshepseg_amd import tilingstats as ts
    seg = np.array(real_raster('seg_final'))
    S = int(seg.max())
    band = np.ones(seg.shape, dtype=np.uint8)
    (ic, _fc) = ts.calcPerSegmentSpatialStats(seg, band, [ts.GFT_Integer], ts.userFuncNumEdgePixels, True, 0, maxSegId=S)
    s = calc(seg, maxSegId=S)
    has = s.columns['area'] > 0
    assert has.sum() > 10
    edge = np.asarray(ic).reshape(-1)
    assert len(edge) == S + 1
    assert np.array_equal(s.columns['edgePixels'][has], edge[has])


# ---- entry points ---------------------------------------------------------------------------------------------------
def test_call_order_is_enforced_and_the_neighbour_table_stays():
    """every refused call fails on the host, before any kernel; shapes leave the context's neighbour table alone"""
    from pyshepseg_amd import _lib, neighbours
    nb = neighbours.findSegmentNeighbours(sc.EXAMPLE, True)
    serial = neighbours.residentTableSerial()
    assert serial is not None and serial == nb.residentSerial
    c = _lib.ctx()
    L = c._L
    table = np.full((1, 11), 7, dtype=np.uint64)
    (S, bad) = (ctypes.c_uint32(0), ctypes.c_uint32(0))

    def finish():
        return L.shp_shape_finish(c.handle, ctypes.byref(S), ctypes.byref(bad), None)

    def refused(rc, what):
        assert rc != 0
        assert what in L.shp_last_error(c.handle).decode()
    calc(sc.EXAMPLE)                                # a finished table: accumulate and finish need a new begin
    refused(L.shp_shape_accumulate_dev(c.handle, None, 1, 1, 0, 0), 'shp_shape_begin must come first')
    refused(finish(), 'shp_shape_begin must come first')
    c.check(L.shp_shape_begin(c.handle, 0, 0, 0))
    refused(L.shp_shape_download(c.handle, _lib.ptr(table)), 'shp_shape_finish must come first')
    assert table.tolist() == [[7] * 11]
    refused(L.shp_shape_begin(c.handle, -1, 0, 0), 'max_seg_id')
    refused(L.shp_shape_begin(c.handle, 0, -1, 0), 'origin')
    refused(L.shp_shape_download(c.handle, _lib.ptr(table)), 'shp_shape_finish must come first')
    c.check(L.shp_shape_begin(c.handle, 0, 0, 0))
    c.check(finish())
    assert (S.value, bad.value) == (0, 0)
    c.check(L.shp_shape_download(c.handle, _lib.ptr(table)))
    assert table.tolist() == [[0] * 11]
    assert neighbours.residentTableSerial() == serial
    out = neighbours.reduceOverNeighbours(nb, [(np.arange(4, dtype=np.float64), [('n', 'count')])])
    assert out['n'].tolist() == [0, 2, 2, 2] and not nb.reduceTimings['uploaded']
    check(sc.EXAMPLE)


def test_readme_example():
    """the two lines of the README: shapes into the column dictionary, then the relative border to other segments"""
    import warnings
    from pyshepseg_amd import neighbours, shapes
    seg = real_raster('mosaic')
    nb = neighbours.findSegmentNeighbours(seg, fourConnected=True)
    cols = dict(nb.columns)
    s = shapes.calcSegmentShapes(seg)
    cols.update(s.columns)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')             # (0 / 0 in the rows of ids without pixels)
        cols['relBorder'] = nb.columns['borderLength'] / cols['perimeter']
    has = cols['area'] > 0
    assert has.any() and np.all((cols['relBorder'][has] >= 0) & (cols['relBorder'][has] <= 1))
    assert np.all(np.isnan(cols['relBorder'][~has]))
    assert np.any(cols['relBorder'][has] < 1)       # the mosaic has label 0 and a rim: some border faces neither
