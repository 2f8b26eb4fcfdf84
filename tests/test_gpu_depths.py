"""GPU: depths.calcSegmentDepths against the numpy model (tests/depth_cases.py, which tests/test_depth_cases_host.py
holds to the literal definition).  Integer arrays are compared with numpy.array_equal, dtype included.  The float
columns are one square root or one division of exact integers each, so they are compared at rtol 1e-12, a generous
bound over one rounding (2^-53).

The kernels (csrc/segdepth.h) work in bands of BAND rows (column step), window tiles of TH x TW pixels that look HALO
columns to either side (row step), patches of PH x TW pixels with a table of SLOTS labels (reduction); a pixel the
window cannot decide goes to the envelope, and ``deferredPixels`` counts those: it must be the number the model of the
window's rule gives (depth_cases.window_deferred), so every case proves which path it took.  Every case runs with
``path='auto'`` and with ``path='envelope'``, and both must give the model's columns and raster.

Not covered: rasters near the pixel limit of 2^32 - 8192 (26 GB of working set and a model to match), and a column
distance beyond 16 bits (more than 131070 rows of one label), whose saturation is argued in the header."""
import ctypes
import functools
import os

import numpy as np
import pytest

import depth_cases as dc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RTOL = 1e-12


def calc(seg, **kw):
    from pyshepseg_amd import depths
    return depths.calcSegmentDepths(seg, **kw)


def assert_columns(got, want, cores=()):
    from pyshepseg_amd import depths
    names = tuple(n for (n, _d) in cores)
    assert sorted(got.columns) == sorted(depths.COUNT_COLUMNS + depths.DERIVED_COLUMNS + names)
    assert got.maxSegId == len(want['maxDepth2']) - 1
    for k in dc.COUNTS + names:
        assert got.columns[k].dtype == np.int64 and np.array_equal(got.columns[k], want[k]), k
    for k in dc.DERIVED:
        assert got.columns[k].dtype == np.float64
        np.testing.assert_allclose(got.columns[k], want[k], rtol=RTOL, atol=0, err_msg=k)
    assert [n for (n, _q) in got.coreAreas] == list(names)
    assert [q for (_n, q) in got.coreAreas] == [int(np.floor(float(d) * float(d))) for (_n, d) in cores]


def check(seg, want_d2=None, cores=(('core1', 1),), origin=(0, 0), maxSegId=None, deferred='model'):
    """both paths against the model's columns and raster (``want_d2``: a closed form that stands in for the model's
    raster); ``deferred``: the count under 'auto', 'model' for depth_cases.window_deferred's"""
    seg = np.asarray(seg)
    if want_d2 is None:
        want_d2 = dc.reference_depth2(seg)
    want = dc.columns_from_depth2(seg, want_d2, cores, origin, maxSegId)
    if deferred == 'model':
        deferred = int(dc.window_deferred(seg).sum())
    out = None
    for path in ('auto', 'envelope'):
        got = calc(seg, coreAreas=cores, origin=origin, maxSegId=maxSegId, depthRaster=True, path=path)
        assert got.depth2.dtype == np.uint32 and got.depth2.shape == seg.shape
        assert np.array_equal(got.depth2, want_d2), path
        assert_columns(got, want, cores)
        assert got.origin == tuple(origin)
        if path == 'auto':
            assert got.deferredPixels == deferred
            out = got
        else:
            assert got.deferredPixels == int(np.count_nonzero(seg))
    return out


# ---- the geometry sweep ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', dc.GEOMETRY, ids=lambda s: '%dx%d' % s)
def test_geometry(shape):
    """1 x 1, a row, a column, 2 x 2, and heights and widths one below, at and one above the tile, band and halo sizes:
    random labels in cells of 1, 5 and 23 pixels, with and without label 0"""
    for seg in dc.geometry_rasters(shape):
        check(seg)


def test_empty_rasters():
    for shape in ((0, 5), (5, 0)):
        got = calc(np.zeros(shape, dtype=np.uint32), maxSegId=2, coreAreas=[('c', 1)], depthRaster=True)
        assert got.columns['maxDepth2'].tolist() == [0, 0, 0] and got.columns['c'].tolist() == [0, 0, 0]
        assert got.columns['maxDepth'].tolist() == [-9999.0] * 3 and got.depth2.shape == shape and got.deferredPixels == 0
    got = calc(np.zeros((3, 3), dtype=np.uint32), depthRaster=True)
    assert got.maxSegId == 0 and not got.depth2.any()


# ---- one label against the closed form ----------------------------------------------------------------------------------
@pytest.mark.parametrize('odd', [True, False], ids=['odd', 'even'])
@pytest.mark.parametrize('depth', [dc.HALO - 1, dc.HALO, dc.HALO + 1], ids=['below', 'at', 'above'])
def test_one_label_square_round_the_halo(depth, odd):
    """the deepest pixel's depth is HALO - 1, HALO, HALO + 1: nothing is deferred up to the halo, something past it; an
    even side's four central pixels tie, and the first in row-major order is reported"""
    seg = dc.square_of_depth(depth, odd)
    side = seg.shape[0]
    got = check(seg, dc.rectangle_depth2(side, side))
    assert (got.deferredPixels == 0) == (depth <= dc.HALO)
    assert got.columns['maxDepth2'][1] == depth * depth
    assert (got.columns['interiorRow'][1], got.columns['interiorCol'][1]) == (depth - 1, depth - 1)


def test_one_label_four_times_the_halo():
    (h, w) = (8 * dc.HALO, 8 * dc.HALO + 10)            # a 2k x 2m rectangle: four central pixels tie
    got = check(dc.one_label(h, w), dc.rectangle_depth2(h, w), cores=(('all', 0), ('deep', 3 * dc.HALO)))
    assert got.columns['maxDepth2'][1] == (4 * dc.HALO) ** 2 and got.deferredPixels > (4 * dc.HALO) ** 2
    assert (got.columns['interiorRow'][1], got.columns['interiorCol'][1]) == (h // 2 - 1, h // 2 - 1)
    assert got.columns['all'][1] == h * w and got.columns['deep'][1] == (h - 6 * dc.HALO) * (w - 6 * dc.HALO)
    assert got.deviceMs > 0 and sorted(got.deviceStepsMs) == sorted(('columns', 'window', 'envelope', 'reduce'))
    assert got.timings['total'] > 0


# ---- thin rasters ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tall', [True, False], ids=['70000x3', '3x70000'])
@pytest.mark.parametrize('nstripes', [1, 3], ids=['one_label', 'stripes'])
def test_thin_rasters(tall, nstripes):
    """column runs of 35000 and more rows, or row runs far longer than the halo, and yet no pixel deeper than 2:
    nothing is deferred"""
    (h, w) = (70000, 3) if tall else (3, 70000)
    seg = dc.stripes(h, w, nstripes, tall)
    got = check(seg, dc.stripes_depth2(h, w, nstripes, tall), deferred=0)
    assert got.columns['maxDepth2'][1:].max() <= 4 and got.maxSegId == nstripes


def test_thin_rasters_across_the_stripes():
    """the other way round: every label one row, or one column, of 70000 pixels"""
    for (h, w, along) in ((3, 70000, True), (70000, 3, False)):
        got = check(dc.stripes(h, w, 3, along), dc.stripes_depth2(h, w, 3, along), deferred=0)
        assert got.columns['maxDepth2'][1:].tolist() == [1, 1, 1]


# ---- shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(dc.SHAPES))
def test_shapes(name):
    """discs and rings inside label 0 and inside another label, with radii round the halo; L, U and comb shapes whose
    nearest foreign pixel lies diagonally; one label in two parts of equal depth; a hole one pixel wide"""
    got = check(dc.shape(name), cores=(('core1', 1), ('core3', 3.2)))
    if name in dc.SHAPES_DEFERRED:
        assert got.deferredPixels > 0
    if name in dc.SHAPES_NOT_DEFERRED:
        assert got.deferredPixels == 0


# ---- the reduction table ------------------------------------------------------------------------------------------------
def test_every_pixel_its_own_label():
    """more labels in a patch than its table has slots: the direct route; every depth2 is 1"""
    seg = dc.every_pixel_its_own()
    got = check(seg, np.ones(seg.shape, dtype=np.uint32), cores=(('all', 0), ('core1', 1)))
    assert np.all(got.columns['maxDepth2'][1:] == 1) and np.all(got.columns['all'][1:] == 1) and not got.columns['core1'].any()


@pytest.mark.parametrize('n', [dc.SLOTS - 1, dc.SLOTS, dc.SLOTS + 1])
def test_labels_round_the_table_slots(n):
    check(dc.labels_in_patch(n), cores=dc.EIGHT_CORES)


def test_sparse_high_ids_and_a_label_above_maxsegid():
    from pyshepseg_amd import depths
    seg = dc.sparse_high_ids()
    top = int(seg.max())
    got = check(seg, maxSegId=top + 1000)
    assert got.maxSegId == top + 1000 and np.count_nonzero(got.columns['maxDepth2']) == len(np.unique(seg)) - 1
    check(seg)
    second = int(np.unique(seg)[-2])
    with pytest.raises(depths.PyShepSegDepthsError, match='segment id %d is above maxSegId %d' % (top, second)):
        calc(seg, maxSegId=second)
    check(dc.u32([[1, 1], [2, 2]]))                     # and the context works on


# ---- arguments and sources ------------------------------------------------------------------------------------------
def test_origin_moves_the_interior_point_and_nothing_else():
    seg = dc.blocky((70, 100), 9, 12, 5, True)
    a = check(seg, cores=dc.EIGHT_CORES)
    b = check(seg, cores=dc.EIGHT_CORES, origin=(1000, 4000000000))
    for k in a.columns:
        moved = {'interiorRow': 1000, 'interiorCol': 4000000000}.get(k, 0)
        has = a.columns['maxDepth2'] > 0
        assert np.array_equal(b.columns[k], a.columns[k] + np.where(has, moved, 0).astype(a.columns[k].dtype)), k


def test_depth_raster_only_on_request_and_eight_cores():
    seg = dc.blocky((90, 150), 17, 6, 11, True)
    (want, d2) = dc.reference_depths(seg, dc.EIGHT_CORES)
    got = calc(seg, coreAreas=dc.EIGHT_CORES)
    assert got.depth2 is None
    assert_columns(got, want, dc.EIGHT_CORES)
    area = np.bincount(seg.ravel(), minlength=got.maxSegId + 1)
    area[0] = 0
    assert np.array_equal(got.columns['core0'], area) and np.array_equal(got.columns['core1'], [(d2[seg == i] > 1).sum() if i else 0
                                                                                            for i in range(got.maxSegId + 1)])
    assert not got.columns['coreMax'].any()
    got = calc(seg, depthRaster=True, missingStatsValue=-1.5, maxSegId=got.maxSegId + 2)
    assert np.array_equal(got.depth2, d2) and not got.depth2[seg == 0].any() and got.columns['maxDepth'][-1] == -1.5


@functools.lru_cache(maxsize=None)
def golden_tile():
    with np.load(os.path.join(GOLDEN, 'tile_synth96_4conn.npz')) as z:
        seg = np.ascontiguousarray(z['seg_final'], dtype=np.uint32)
    seg.setflags(write=False)
    return seg


class Resident(object):
    """labels in device memory, as a segmentation kept on the device hands them over (``outDev``)"""
    def __init__(self, seg):
        from pyshepseg_amd import _lib
        self.c = _lib.ctx()
        self.p = ctypes.c_void_p()
        self.c.check(self.c._L.shp_dev_alloc(self.c.handle, seg.nbytes, ctypes.byref(self.p)))
        self.c.check(self.c._L.shp_dev_upload(self.c.handle, self.p, seg.ctypes.data_as(ctypes.c_void_p), seg.nbytes))
        self.outDev = (self.p.value, seg.shape[0], seg.shape[1], seg.nbytes)
        self.maxSegId = None

    def free(self):
        self.c.check(self.c._L.shp_dev_free(self.c.handle, self.p))


def test_sources_give_one_result(tmp_path):
    """host array, .npy path, a result object with its own maxSegId, labels resident in HBM"""
    from pyshepseg_amd import tiling
    seg = golden_tile()
    cores = (('core0', 0), ('core1', 1))
    (want, d2) = dc.reference_depths(seg, cores)
    path = str(tmp_path / 'labels.npy')
    np.save(path, seg)
    res = tiling.TiledSegmentationResult()
    res.segimg = seg
    res.maxSegId = int(seg.max())
    dev = Resident(seg)
    try:
        for src in (seg, path, res, dev):
            got = calc(src, coreAreas=cores, depthRaster=True)
            assert_columns(got, want, cores)
            assert np.array_equal(got.depth2, d2)
    finally:
        dev.free()


def test_cores_against_the_shape_columns():
    from pyshepseg_amd import shapes
    seg = golden_tile()
    got = calc(seg, coreAreas=(('core0', 0), ('core1', 1)), depthRaster=True)
    shp = shapes.calcSegmentShapes(seg)
    assert np.array_equal(got.columns['core0'], shp.columns['area'])
    assert np.array_equal(got.columns['core1'], shp.columns['area'] - shp.columns['edgePixels'])
    assert np.array_equal(np.bincount(seg[got.depth2 == 1].astype(np.int64), minlength=got.maxSegId + 1), shp.columns['edgePixels'])


def _inside(ring2, py, px):
    """even-odd crossing count in doubled integer coordinates: a ray from (py, px) towards increasing column against
    the ring's vertical segments"""
    nxt = np.roll(ring2, -1, axis=0)
    vertical = ring2[:, 1] == nxt[:, 1]
    lo = np.minimum(ring2[:, 0], nxt[:, 0])
    hi = np.maximum(ring2[:, 0], nxt[:, 0])
    return bool(np.count_nonzero(vertical & (ring2[:, 1] > px) & (lo < py) & (py < hi)) & 1)


def test_interior_point_lies_in_a_polygon_and_the_rings_stay_resident():
    """the centre of every id's interior pixel lies inside one of its polygons: inside the shell and in none of its
    holes; and the trace's rings are still the resident ones after the depths, so the hulls read them in place"""
    from pyshepseg_amd import outlines
    seg = golden_tile()
    o = outlines.traceSegmentOutlines(seg, origin=(7, 11))
    serial = outlines.residentOutlineSerial()
    assert serial is not None and serial == o.residentSerial
    got = calc(seg, origin=(7, 11))
    assert outlines.residentOutlineSerial() == serial
    hulls = outlines.calcSegmentHulls(o)
    assert not hulls.timings['uploaded']
    ids = [i for i in range(1, got.maxSegId + 1) if got.columns['maxDepth2'][i] > 0]
    assert len(ids) == len(np.unique(seg[seg != 0]))
    for i in ids:
        (py, px) = (2 * int(got.columns['interiorRow'][i]) + 1, 2 * int(got.columns['interiorCol'][i]) + 1)
        assert seg[(py - 1) // 2 - 7, (px - 1) // 2 - 11] == i
        hits = 0
        for poly in o.polygonsOf(i):
            if _inside(2 * poly[0], py, px) and not any(_inside(2 * hole, py, px) for hole in poly[1:]):
                hits += 1
        assert hits == 1, i


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_working_set_is_sized_and_refused_before_it_is_allocated(monkeypatch):
    """shp_depth_need's bytes (6 a pixel, 20 per column and band, 12 per piece of a row, 88 an id, 16 per 65 pixels, each buffer with the eighth
    the context's buffers grow by; 8 per scratch position); a call that does not fit the free memory raises with the
    bytes named before the labels go up, and before the envelope's scratch when that does not fit"""
    from pyshepseg_amd import _lib, depths
    c = _lib.ctx()
    (need, free) = (ctypes.c_int64(0), ctypes.c_int64(0))
    (nrows, ncols, S) = (3 * 2 ** 15, 2 ** 15, 10 ** 6)
    npix = nrows * ncols
    c.check(c._L.shp_depth_need(c.handle, nrows, ncols, S, 0, -1, ctypes.byref(need), ctypes.byref(free)))
    exact = (6 * npix + 20 * (nrows // dc.BAND) * ncols + 12 * nrows * (ncols // dc.TW) + 88 * (S + 1) +
             16 * (npix // (2 * dc.HALO + 1) + 1))
    assert exact <= need.value <= exact * 9 // 8 + 2 ** 20 and free.value > 2 ** 30
    c.check(c._L.shp_depth_need(c.handle, nrows, ncols, S, 1, -1, ctypes.byref(need), ctypes.byref(free)))
    assert need.value >= 22 * npix
    c.check(c._L.shp_depth_need(c.handle, nrows, ncols, S, 0, 2 ** 31, ctypes.byref(need), ctypes.byref(free)))
    assert 8 * 2 ** 31 <= need.value <= 9 * 2 ** 31 + 2 ** 20
    assert c._L.shp_depth_need(c.handle, 2 ** 16, 2 ** 16, S, 0, -1, ctypes.byref(need), ctypes.byref(free)) != 0

    class Library(object):
        """the library, whose buffers would have to grow by a terabyte more from the (after + 1)-th question on"""
        def __init__(self, after):
            (self.after, self.calls) = (after, [])

        def __getattr__(self, name):
            fn = getattr(c._L, name)

            def call(*args):
                self.calls.append(name)
                rc = fn(*args)
                if name == 'shp_depth_need' and self.calls.count(name) > self.after:
                    args[6]._obj.value += 10 ** 12
                return rc
            return call

    class Ctx(object):
        def __init__(self, after):
            (self.handle, self.check, self._L) = (c.handle, c.check, Library(after))

    seg = dc.square_of_depth(dc.HALO + 1)
    fake = Ctx(0)
    monkeypatch.setattr(_lib, 'ctx', lambda: fake)
    with pytest.raises(depths.PyShepSegDepthsError, match=r'65 x 65 pixels need 1\d{12} bytes of device memory, \d+ are free'):
        calc(seg, maxSegId=1)
    assert fake._L.calls == ['shp_depth_need']
    fake = Ctx(1)
    with pytest.raises(depths.PyShepSegDepthsError, match=r'2 ids need 1\d{12} bytes of device memory, \d+ are free'):
        calc(seg)
    assert 'shp_depth_transform_dev' not in fake._L.calls
    fake = Ctx(1)
    with pytest.raises(depths.PyShepSegDepthsError, match=r'scratch of 67 positions needs 1\d{12} bytes of device memory, \d+ are free'):
        calc(seg, maxSegId=1)
    assert 'shp_depth_envelope' not in fake._L.calls and fake._L.calls[-2:] == ['shp_depth_need', 'shp_dev_free']
    monkeypatch.undo()
    check(seg, dc.rectangle_depth2(*seg.shape))


def test_call_order_is_enforced():
    from pyshepseg_amd import _lib
    c = _lib.ctx()
    L = c._L
    check(dc.u32([[1, 1], [2, 0]]))
    table = np.zeros((3, 11), dtype=np.uint64)
    c.check(L.shp_depth_download(c.handle, _lib.ptr(table), None))
    assert table[:, 0].tolist() == [0, 2, 1]
    bad = ctypes.c_uint32(0)
    for (call, text) in ((lambda: L.shp_depth_envelope(c.handle), 'shp_depth_transform_dev must come first'),
                         (lambda: L.shp_depth_reduce(c.handle, 2, 0, None, ctypes.byref(bad), None),
                          'shp_depth_envelope must come first')):
        with pytest.raises(_lib.ShepsegHipError, match=text):
            c.check(call())
    counts = np.zeros(3, dtype=np.int64)
    c.check(L.shp_depth_transform_dev(c.handle, None, 0, 0, 0, _lib.ptr(counts)))
    rc = L.shp_depth_download(c.handle, _lib.ptr(table), None)
    with pytest.raises(_lib.ShepsegHipError, match='shp_depth_reduce must come first'):
        c.check(rc)
    check(dc.u32([[1, 1], [2, 0]]))


def test_readme_example(tmp_path):
    """the README's lines: the depth columns into the column dictionary, the interior point out as GeoJSON properties"""
    import json
    import math
    from pyshepseg_amd import depths, outlines, shapes
    seg = golden_tile()
    o = outlines.traceSegmentOutlines(seg)
    cols = dict(shapes.calcSegmentShapes(seg).columns)
    d = depths.calcSegmentDepths(seg, coreAreas=[('coreArea2', 2.0)])
    cols.update(d.columns)
    ids = np.argsort(cols['area'])[-3:]
    path = str(tmp_path / 'seg.geojson')
    assert outlines.writeGeoJSON(o, path, ids=ids, columns=cols) == 3
    with open(path) as f:
        feats = json.load(f)['features']
    for f in feats:
        p = f['properties']
        assert seg[p['interiorRow'], p['interiorCol']] == p['segId'] and p['coreArea2'] <= p['area'] - p['edgePixels']
        assert p['maxDepth'] == math.sqrt(p['maxDepth2'])
