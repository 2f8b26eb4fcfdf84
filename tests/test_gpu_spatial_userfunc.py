"""GPU: user-defined spatial statistics -- the per-segment point lists of iterSegmentPoints in the reference's
visit order, and calcPerSegmentSpatialStats(Tiled) with plain-Python user functions (spatialUserFunc) against the reference's
golden vectors and the oracle."""
import ctypes

import numpy as np
import pytest

import segpoints_helpers as H

pytestmark = pytest.mark.gpu


def _raster(dtype, seed=7, shape=(2000, 1800)):
    """Irregular blocks of 1..S with holes: 2 % of pixels unlabelled, 5 % nodata, a few segments all nodata, ids
    without pixels (the largest ids and some in between)."""
    rng = np.random.RandomState(seed)
    base = rng.permutation(np.arange(1, 41 * 37 + 1)).reshape(41, 37).astype(np.uint32)
    seg = np.kron(base, np.ones((53, 51), dtype=np.uint32))[:shape[0], :shape[1]].copy()
    seg[rng.rand(*seg.shape) < 0.02] = 0
    seg[(seg % 97) == 5] = 0                                 # ids without pixels
    info = np.iinfo(dtype)
    band = rng.randint(max(info.min, -30000), min(info.max, 60000) + 1, size=seg.shape).astype(dtype)
    null = 0 if info.min == 0 else -1
    band[band == null] = 1
    band[rng.rand(*seg.shape) < 0.05] = null
    band[(seg % 89) == 3] = null                             # all-nodata segments
    return seg, band, null


def _collect(batches):
    ids, offs, x, y, val = [], [], [], [], []
    total = 0
    for (bid, off, pts) in batches:
        assert off[0] == 0 and len(off) == len(bid) + 1 and off[-1] == len(pts)
        ids.append(np.asarray(bid).copy())
        offs.append(off[1:] + total)
        total += len(pts)
        x.append(np.array(pts.x))
        y.append(np.array(pts.y))
        val.append(np.array(pts.val))
    cat = np.concatenate
    return cat(ids), cat([[0]] + offs), cat(x), cat(y), cat(val)


def _check_against_numpy(got, seg, band, null, tile, S):
    (ids, offs, x, y, val) = got
    assert np.array_equal(ids, np.arange(1, S + 1))
    (wid, wx, wy, wv) = H.visit_points(seg, band, null, tile, S)
    assert np.array_equal(np.diff(offs), np.bincount(wid, minlength=S + 1)[1:])
    assert np.array_equal(x, wx) and np.array_equal(y, wy) and np.array_equal(val, wv)


CASES = [(1024, np.uint16), (48, np.uint16), (37, np.uint16), (37, np.uint8), (48, np.int16), (37, np.uint32),
         (1024, np.int32)]


@pytest.mark.parametrize('tile,dtype', CASES)
def test_iter_points_visit_order(tile, dtype):
    from pyshepseg_amd import tilingstats as ts
    (seg, band, null) = _raster(dtype)
    S = int(seg.max()) + 3
    batches = list(ts.iterSegmentPoints(seg, band, null, tileSize=tile, maxSegId=S))
    assert len(batches) == 1 and not batches[0][2].flags.writeable and not batches[0][1].flags.writeable
    got = _collect(batches)
    _check_against_numpy(got, seg, band, null, tile, S)
    assert got[4].dtype == np.int64


def test_iter_points_small_batches_equal_one_batch():
    from pyshepseg_amd import tilingstats as ts
    (seg, band, null) = _raster(np.uint16, seed=9, shape=(700, 650))
    S = int(seg.max())
    one = [(b.copy(), o.copy(), p.copy()) for (b, o, p) in
           ts.iterSegmentPoints(seg, band, null, tileSize=37, batchPoints=1 << 30)]
    assert len(one) == 1
    ref = _collect(one)
    counts = np.bincount(seg[(seg != 0) & (band != null)], minlength=S + 1)
    budget = int(np.median(counts[counts > 0]))             # about half the segments are larger: batches of one
    nb = 0
    parts = []
    for (bid, off, pts) in ts.iterSegmentPoints(seg, band, null, tileSize=37, batchPoints=budget):
        nb += 1
        if len(pts) > budget:
            assert (np.diff(off) > 0).sum() == 1
        parts.append((bid.copy(), off.copy(), pts.copy()))
    assert nb > 100
    got = _collect(parts)
    for (a, b) in zip(got, ref):
        assert np.array_equal(a, b)
    _check_against_numpy(got, seg, band, null, 37, S)


def test_batches_outlive_the_generator():
    """list(iterSegmentPoints(...)) keeps batches whose memory was reused, but never freed memory: the last two
    batches still hold their own points."""
    from pyshepseg_amd import tilingstats as ts
    (seg, band, null) = _raster(np.uint8, seed=4, shape=(300, 280))
    S = int(seg.max())
    kept = list(ts.iterSegmentPoints(seg, band, null, tileSize=48, batchPoints=2000))
    assert len(kept) > 4
    (wid, wx, wy, _wv) = H.visit_points(seg, band, null, 48, S)
    for (bid, off, pts) in kept[-2:]:
        sel = (wid >= bid[0]) & (wid <= bid[-1])
        assert np.array_equal(pts.x, wx[sel]) and np.array_equal(pts.y, wy[sel])


def test_segpoints_host_entry_points():
    """shp_segpoints_count / _build / _emit with host rasters; emit errors without a build and with a short buffer."""
    from pyshepseg_amd import _lib
    (seg, band, null) = _raster(np.int16, seed=3, shape=(300, 260))
    S = int(seg.max())
    c = _lib.Context()
    try:
        L = c._L
        dt = _lib.SHP_DTYPES[band.dtype]
        counts = np.zeros(S + 1, np.uint32)
        c.check(L.shp_segpoints_count(c.handle, _lib.ptr(seg), _lib.ptr(band), dt, 300, 260, S, null,
                                      _lib.ptr(counts)))
        assert np.array_equal(counts, np.bincount(seg[(seg != 0) & (band != null)], minlength=S + 1))
        offs = np.zeros(S + 2, np.int64)
        n = ctypes.c_int64(0)
        with pytest.raises(_lib.ShepsegHipError, match='shp_segpoints_build'):
            c.check(L.shp_segpoints_emit(c.handle, 1, S + 1, _lib.ptr(offs), None, 0, ctypes.byref(n)))
        npts = ctypes.c_int64(0)
        c.check(L.shp_segpoints_build(c.handle, _lib.ptr(seg), _lib.ptr(band), dt, 300, 260, S, null, 64,
                                      ctypes.byref(npts)))
        assert npts.value == counts.sum()
        with pytest.raises(_lib.ShepsegHipError, match='points'):
            c.check(L.shp_segpoints_emit(c.handle, 1, S + 1, _lib.ptr(offs), _lib.ptr(offs), 10, ctypes.byref(n)))
        assert n.value == counts.sum()
        pts = np.zeros(n.value, dtype=[('x', np.uint32), ('y', np.uint32), ('val', np.int64)])
        c.check(L.shp_segpoints_emit(c.handle, 0, S + 1, _lib.ptr(offs), _lib.ptr(pts), len(pts), ctypes.byref(n)))
        (wid, wx, wy, wv) = H.visit_points(seg, band, null, 64, S)
        assert np.array_equal(offs, np.concatenate([[0], np.cumsum(counts)]))
        assert np.array_equal(pts['x'], wx) and np.array_equal(pts['y'], wy) and np.array_equal(pts['val'], wv)
        with pytest.raises(_lib.ShepsegHipError, match='id range'):
            c.check(L.shp_segpoints_emit(c.handle, 5, S + 2, _lib.ptr(offs), _lib.ptr(pts), len(pts),
                                         ctypes.byref(n)))
    finally:
        c.close()


def _golden_cases(g):
    from pyshepseg_amd import tilingstats as ts
    R, I = ts.GFT_Real, ts.GFT_Integer
    return [('mean_fc', H.mean_coord, g['transform'], [('e', R), ('n', R)]),
            ('meanrot_fc', H.mean_coord, g['rot'], [('e', R), ('n', R)]),
            ('edge4_ic', H.num_edge_pixels, True, [('edges', I)]),
            ('edge8_ic', H.num_edge_pixels, False, [('edges', I)]),
            ('vario_fc', H.variogram, 4, [('v%d' % i, R) for i in range(4)])]


def test_golden_python_user_functions(golden):
    """Plain-Python versions of the reference's three examples, fed the GPU's point lists: bit-equal to the
    reference's own njit results for every segment (mean coordinates included: the points come in its order)."""
    from pyshepseg_amd import tilingstats as ts
    g = golden('spatial_stats')
    assert int(g['tile']) == 48
    for key, fn, prm, cols in _golden_cases(g):
        r = ts.calcPerSegmentSpatialStatsTiled(g['band'], 1, g['seg'], cols, ts.spatialUserFunc(fn), prm,
                                               imgNullVal=int(g['null_val']),
                                               tileSize=48)
        got = np.stack([r.columns[n] for (n, _t) in cols])
        want = g[key]
        assert got.dtype == want.dtype
        if got.dtype == np.float32:
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), key
        else:
            assert np.array_equal(got, want), key


def test_python_mean_coord_vs_oracle(oracle):
    """A rotated, non-integer geotransform on a raster wider and taller than one 1024 tile: the per-point float64
    sums of a Python callback equal the oracle's (the reference's order) bit for bit."""
    from pyshepseg_amd import tilingstats as ts
    (seg, band, null) = _raster(np.uint16, seed=13, shape=(1300, 1150))
    S = int(seg.max())
    rot = np.array([1000.5, 10.0, 0.25, -2000.25, -0.5, -10.0])
    R = ts.GFT_Real
    _ic, fc = ts.calcPerSegmentSpatialStats(seg, band, [R, R], ts.spatialUserFunc(H.mean_coord_vec), rot, null)
    _wi, wf = oracle.spatialstats(seg, band, 'meancoord', rot, null, 0, 2, max_seg_id=S, tile_size=1024)
    assert np.array_equal(fc.view(np.uint32), wf.view(np.uint32))
    # the built-in sums re-associate: the Python callback is the one that follows the reference's order
    _ic, fb = ts.calcPerSegmentSpatialStats(seg, band, [R, R], ts.userFuncMeanCoord, rot, null)
    assert np.allclose(fb, wf, rtol=1e-6, atol=0)


def test_user_function_errors_and_partial_columns():
    from pyshepseg_amd import tilingstats as ts
    (seg, band, null) = _raster(np.uint16, seed=5, shape=(200, 180))
    S = int(seg.max())
    R, I = ts.GFT_Real, ts.GFT_Integer

    class Boom(Exception):
        pass

    @ts.spatialUserFunc
    def bad(pts, nullv, intArr, floatArr, prm):
        if pts.y.max() > 100:
            raise Boom('segment at row %d' % pts.y.max())
    with pytest.raises(Boom, match='segment at row'):
        ts.calcPerSegmentSpatialStatsTiled(band, 1, seg, [('a', R)], bad, None, imgNullVal=null)

    @ts.spatialUserFunc
    def one_col(pts, nullv, intArr, floatArr, prm):
        intArr[0] = len(pts) + prm
    r = ts.calcPerSegmentSpatialStatsTiled(band, 1, seg, [('n', I), ('m', I), ('f', R)], one_col, 1000,
                                           missingStatsValue=-5, imgNullVal=null, tileSize=37)
    counts = np.bincount(seg[(seg != 0) & (band != null)], minlength=S + 1)
    has = counts > 0
    has[0] = False
    assert r.columns['n'].dtype == np.int64 and r.columns['f'].dtype == np.float32
    assert np.array_equal(r.columns['n'][has], counts[has] + 1000)
    assert (r.columns['n'][1:][~has[1:]] == -5).all()
    assert (r.columns['m'][1:] == -5).all() and (r.columns['f'][1:] == -5).all()
    assert r.columns['n'][0] == 0 and r.columns['m'][0] == 0 and r.columns['f'][0] == 0


def test_decorated_lambda_runs():
    """An undecorated callable is refused (tests/test_gpu_stats.py); the same lambda decorated with
    spatialUserFunc runs, and leaves its column at missing."""
    from pyshepseg_amd import tilingstats as ts
    seg = np.ones((8, 8), np.uint32)
    img = np.ones((8, 8), np.uint16)
    r = ts.calcPerSegmentSpatialStatsTiled(img, 1, seg, [('a', ts.GFT_Real)], ts.spatialUserFunc(lambda *a: None),
                                           None, imgNullVal=0)
    assert r.columns['a'].tolist() == [0.0, -9999.0]
