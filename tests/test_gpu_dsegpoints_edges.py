"""GPU: the point lists of row shards (csrc/dsegpoints.h) at their slice, record, share and value edges, on one GPU
with the thread ranks of spatial_dist_helpers.runShards.  Every rank's columns of the order-sensitive order_hash equal,
bit for bit, runUserFunc over numpy_batches of the whole raster and the one-GPU call; the points every call was handed
equal visit_points of the whole raster.  The last test drives shp_dsegpoints_build_dev / _merge_dev / _emit directly,
on two shards of a raster whose visit indices pass 2^32.  tests/test_segpoints_cases_host.py proves that each case
reaches the edge it is named for."""
import ctypes

import numpy as np
import pytest

import segpoints_cases as C
import segpoints_helpers as P
import spatial_dist_helpers as H
import spatial_userfunc_dist_helpers as U

pytestmark = pytest.mark.gpu

PARAM = 9


def _types():
    from pyshepseg_amd import tilingstats as ts
    return [ts.GFT_Integer, ts.GFT_Real, ts.GFT_Integer, ts.GFT_Real]


def _same(a, b):
    return (a[0].dtype == b[0].dtype and a[1].dtype == b[1].dtype and np.array_equal(a[0], b[0]) and
            np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


_want = {}


def want(name, case):
    """(one-GPU columns == the numpy restatement fed to the same function, visit_points): once per named case"""
    if name not in _want:
        from pyshepseg_amd import tilingstats as ts
        (seg, band, null, S, tile) = case
        fn = ts.spatialUserFunc(U.order_hash)
        one = ts.calcPerSegmentSpatialStats(seg, band, _types(), fn, PARAM, null, maxSegId=S, tileSize=tile)
        nump = ts.runUserFunc(P.numpy_batches(seg, band, null, tile, [(1, S + 1)], S), S + 1, fn, PARAM, null, 2, 2)
        assert _same(one, nump)
        _want[name] = (one, P.visit_points(seg, band, null, tile, S))
    return _want[name]


def check_split(name, case, cuts, batch=None):
    """deviceSpatialStats on the row shards `cuts`; returns every rank's info"""
    from pyshepseg_amd import distributed, _lib, tilingstats as ts
    (seg, band, null, S, tile) = case
    (nr, nc) = seg.shape
    world = len(cuts)
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
    hist[0] = 0
    seen = [{} for _r in range(world)]

    def work(c, comm, d_seg, d_band, rr):
        def fn(pts, nullv, intArr, floatArr, prm):
            i = int(seg[int(pts.y[0]), int(pts.x[0])])
            assert i not in seen[comm.rank]
            seen[comm.rank][i] = (np.array(pts.x), np.array(pts.y), np.array(pts.val))
            U.order_hash(pts, nullv, intArr, floatArr, prm)
        info = {}
        res = distributed.deviceSpatialStats(c, comm, d_seg, d_band, _lib.SHP_DTYPES[band.dtype], nr, nc, rr, hist,
                                             _types(), ts.spatialUserFunc(fn), PARAM, -9999, null, tileSize=tile,
                                             batchPoints=batch, info=info)
        return res, info
    (results, errors) = H.runShards(seg, band, cuts, work, timeout=120)
    assert not any(errors), errors
    (one, (wid, wx, wy, wv)) = want(name, case)
    for r in range(world):
        assert _same(results[r][0][:2], one), r
    # every id with points was handed, once and on one rank, exactly the whole raster's points in visit order
    held = [set(np.unique(seg[a:b]).tolist()) - {0} for (a, b) in cuts]
    strad = set()
    for i in range(world):
        for j in range(i + 1, world):
            strad |= held[i] & held[j]
    starts = np.searchsorted(wid, np.arange(S + 2))
    called = {}
    for r in range(world):
        (lo, hi) = distributed.idRange(r, world, S)
        for (i, (x, y, v)) in seen[r].items():
            assert i not in called, i
            called[i] = r
            assert (lo <= i < hi) if i in strad else (i in held[r]), (i, r)
            sl = slice(starts[i], starts[i + 1])
            assert v.dtype == np.int64 and np.array_equal(v, wv[sl]), (i, r)
            assert np.array_equal(x, wx[sl]) and np.array_equal(y, wy[sl]), (i, r)
    assert sorted(called) == np.unique(wid).tolist()
    valid = (seg != 0) & (seg <= S) & (band.astype(np.int64) != int(null))
    exchanged = int(np.isin(seg[valid], sorted(strad)).sum()) if strad else 0
    infos = [res[1] for res in results]
    for info in infos:
        assert info['path'] == 'points' and info['points_exchanged'] == exchanged
        assert info['straddlers'] == len(strad)
    return infos, strad, exchanged


# ---- slices ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tile', C.SLICE_TILES)
@pytest.mark.parametrize('cut', sorted(C.SLICE_CUTS))
def test_slices(cut, tile):
    ((seg, band, null, S, _t), _p) = C.slice_raster(70)
    (_i, strad, _e) = check_split('slice-70-%d' % tile, (seg, band, null, S, tile), C.SLICE_CUTS[cut],
                                  batch=200 if tile == 8 else None)
    assert len(strad) >= 6


@pytest.mark.parametrize('cut', ['row-after', 'inside-one-band', 'empty-middle'])
def test_slices_last_tile_column_one_wide(cut):
    ((seg, band, null, S, _t), _p) = C.slice_raster(129)
    check_split('slice-129-128', (seg, band, null, S, 128), C.SLICE_CUTS[cut])


# ---- records -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cuts', [[(0, 20), (20, 40)], [(0, 13), (13, 27), (27, 40)]])
def test_records_past_one_scan_block(cuts):
    (case, p) = C.records_one_id()
    (_i, strad, exchanged) = check_split('records_one_id', case, cuts)
    assert strad == {1} and exchanged == p['records'] > C.SCAN_BLOCK


@pytest.mark.parametrize('cuts', [[(0, 20), (20, 40)], [(0, 9), (9, 10), (10, 40)]])
def test_records_every_id_a_straddler(cuts):
    (case, _p) = C.records_stripes()
    (_i, strad, exchanged) = check_split('records_stripes', case, cuts, batch=500)
    assert len(strad) == case[3] and exchanged == 12000


def test_records_none():
    (case, p) = C.records_bands()
    (_i, strad, exchanged) = check_split('records_bands', case, p['cuts'])
    assert not strad and exchanged == 0


def test_records_complete_and_straddler_runs_alternate():
    (case, p) = C.records_alternating()
    (_i, strad, _e) = check_split('records_alternating', case, p['cuts'])
    assert len(strad) == 75
    check_split('records_alternating', case, p['cuts'], batch=700)


# ---- shares ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('world,S', C.SHARE_CASES)
def test_shares(world, S):
    (case, p) = C.shares(world, S)
    (_i, strad, _e) = check_split('shares-%d-%d' % (world, S), case, p['cuts'])
    assert sorted(strad) == p['straddlers']


# ---- values through the exchange ---------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', C.DTYPES)
def test_values_through_the_exchange(dtype):
    """every id a straddler: each value is cut to 32 bits, travels, and arrives as itself"""
    nulls = C.value_nulls(dtype)
    for null in (nulls[0], nulls[1], nulls[-1]):
        (case, p) = C.values(dtype, null, stripes=True)
        (_i, strad, _e) = check_split('values-%s-%d' % (np.dtype(dtype).name, null), case, [(0, 2), (2, 5)])
        assert len(strad) == 6
        (_one, (_wid, _wx, _wy, wv)) = want('values-%s-%d' % (np.dtype(dtype).name, null), case)
        assert set(wv.tolist()) == set(p['values'].tolist()) - {null}


# ---- visit indices of 2^32 and above -----------------------------------------------------------------------------
def test_visit_indices_past_2_pow_32():
    """Two 4-row shards of the last band of a 65536 x 65537 raster, one rank after the other in one thread: the
    straddler's records carry 64-bit visit indices on both sides of 2^32, and the owner's merge needs the sort pass
    over their high word to emit them in visit order."""
    from pyshepseg_amd import _lib, distributed
    B = C.BIG
    (S, R, T, world) = (B['S'], B['img_rows'], B['tile'], 2)
    (shards, hist) = C.big_visit_shards()
    pts = [C.visit_points(s, b, 0, T, S, row0=lo, img_rows=R, with_key=True) for (s, b, lo) in shards]
    cc = _lib.Context()                                     # the copies' context: the ranks' contexts keep their lists
    pcs = [_lib.Context() for _r in range(world)]
    L = cc._L
    bufs = []

    def up(a):
        p = ctypes.c_void_p()
        cc.check(L.shp_dev_alloc(cc.handle, a.nbytes, ctypes.byref(p)))
        bufs.append(p)
        cc.check(L.shp_dev_upload(cc.handle, p, _lib.ptr(a), a.nbytes))
        return p
    try:
        d_hist = up(hist)
        recs = []
        for (r, (seg, band, lo)) in enumerate(shards):
            (lh, lp) = (np.zeros(S + 1, np.uint32), np.zeros(S + 1, np.uint32))
            (pRec, nRec) = (ctypes.c_void_p(), ctypes.c_int64(-1))
            pcs[r].check(L.shp_dsegpoints_build_dev(
                pcs[r].handle, up(seg), up(band), _lib.SHP_DTYPES[band.dtype], seg.shape[0], seg.shape[1], lo, R, S,
                0, T, d_hist, _lib.ptr(lh), _lib.ptr(lp), ctypes.byref(pRec), ctypes.byref(nRec)))
            (ids, x, y, val, key) = pts[r]
            assert np.array_equal(lh, np.bincount(seg.ravel(), minlength=S + 1)[:S + 1] * (np.arange(S + 1) > 0))
            assert np.array_equal(lp, np.bincount(ids, minlength=S + 1))
            one = ids == 1
            assert nRec.value == one.sum() == 60
            rec = np.zeros((nRec.value, 3), dtype=np.uint64)
            cc.check(L.shp_dev_download(cc.handle, _lib.ptr(rec), pRec, rec.nbytes))
            # the records as they travel: {visit index; id | x << 32; y | value bits << 32}
            assert np.array_equal(rec[:, 0], key[one].astype(np.uint64))
            assert np.array_equal(rec[:, 1], (1 + (x[one] << 32)).astype(np.uint64))
            assert np.array_equal(rec[:, 2], (y[one] + (val[one] << 32)).astype(np.uint64))
            recs.append(rec)
        counts = np.array([len(q) for q in recs], dtype=np.uint32)
        slot = int(counts.max())
        gathered = np.zeros((world, slot, 3), dtype=np.uint64)
        for (r, q) in enumerate(recs):
            gathered[r, :len(q)] = q
        d_all = up(gathered)
        cat = [np.concatenate([p[k][p[0] == 1] for p in pts]) for k in range(5)]
        order = np.argsort(cat[4], kind='stable')
        assert cat[4][order][0] < 2 ** 32 <= cat[4][order][-1]
        for r in range(world):
            (lo, hi) = distributed.idRange(r, world, S)
            merged = np.full(max(hi - lo, 1), 0xEEEEEEEE, dtype=np.uint32)
            nm = ctypes.c_int64(-1)
            pcs[r].check(L.shp_dsegpoints_merge_dev(pcs[r].handle, d_all, slot, world, _lib.ptr(counts), lo, hi,
                                                    _lib.ptr(merged), ctypes.byref(nm)))
            owner = lo <= 1 < hi
            assert owner == (r == 0) and nm.value == (120 if owner else 0)
            assert merged[:hi - lo].tolist() == [120 if i == 1 else 0 for i in range(lo, hi)]
            # the expected emission: the straddler from the merge on its owner, the complete id from the local runs
            (ids, x, y, val, _key) = pts[r]
            mine = ids == 2 + r
            parts = ([tuple(c[order] for c in cat[1:4])] if owner else []) + [(x[mine], y[mine], val[mine])]
            (wx, wy, wv) = (np.concatenate([p[k] for p in parts]) for k in range(3))
            woffs = np.zeros(S + 2, dtype=np.int64)
            woffs[2:] += 120 if owner else 0
            woffs[3 + r:] += mine.sum()
            n = ctypes.c_int64(-1)
            offs = np.full(S + 2, -7, dtype=np.int64)
            out = np.zeros(len(wx), dtype=[('x', np.uint32), ('y', np.uint32), ('val', np.int64)])
            pcs[r].check(L.shp_dsegpoints_emit(pcs[r].handle, 0, S + 1, _lib.ptr(offs), _lib.ptr(out), len(out),
                                               ctypes.byref(n)))
            assert n.value == len(wx) and np.array_equal(offs, woffs)
            assert np.array_equal(out['x'], wx) and np.array_equal(out['y'], wy) and np.array_equal(out['val'], wv)
            assert out['y'].min() >= B['rows'][0][0]           # y is the row of the whole raster
    finally:
        for p in bufs:
            L.shp_dev_free(cc.handle, p)
        for c in pcs + [cc]:
            c.close()


def test_tile_row_reaching_2_pow_32_pixels():
    """A 2 x 2 shard at row 2^31 - 1 of a raster 2^31 + 10 rows high and 2 wide.  Tile 2^31: a tile row holds 2^32
    pixels and is not the only one -- refused on every rank before any launch, by return code and message
    (pts_visit_pos divides by a tile row's pixels in 32 bits).  Tile 2^31 - 1: the shard starts a tile row of 2^32 - 2
    pixels; its points come back in visit order, y the row of the whole raster (2^31 - 1 and 2^31)."""
    from pyshepseg_amd import _lib
    seg = np.array([[1, 2], [2, 1]], dtype=np.uint32)
    band = np.array([[5, 6], [7, 8]], dtype=np.uint16)
    hist = np.array([0, 2, 2], dtype=np.uint32)
    (R, row0, S) = (2 ** 31 + 10, 2 ** 31 - 1, 2)
    cc = _lib.Context()
    pc = _lib.Context()
    L = cc._L
    bufs = []
    try:
        ptrs = []
        for a in (seg, band, hist):
            p = ctypes.c_void_p()
            cc.check(L.shp_dev_alloc(cc.handle, a.nbytes, ctypes.byref(p)))
            bufs.append(p)
            cc.check(L.shp_dev_upload(cc.handle, p, _lib.ptr(a), a.nbytes))
            ptrs.append(p)
        (lh, lp) = (np.zeros(S + 1, np.uint32), np.zeros(S + 1, np.uint32))
        (pRec, nRec) = (ctypes.c_void_p(), ctypes.c_int64(-1))

        def build(tile):
            return L.shp_dsegpoints_build_dev(pc.handle, ptrs[0], ptrs[1], _lib.SHP_DTYPES[band.dtype], 2, 2, row0, R,
                                              S, 0, tile, ptrs[2], _lib.ptr(lh), _lib.ptr(lp), ctypes.byref(pRec),
                                              ctypes.byref(nRec))
        for tile in (2 ** 31, 2 ** 31 + 5):
            assert build(tile) == -3                        # SHP_ERR_ARG
            msg = L.shp_last_error(pc.handle).decode()
            assert 'a tile row of %d x 2 px reaches 2^32 pixels' % tile in msg and nRec.value == -1
        tile = 2 ** 31 - 1
        pc.check(build(tile))
        assert nRec.value == 0 and lh.tolist() == [0, 2, 2] and lp.tolist() == [0, 2, 2]
        (merged, nm) = (np.zeros(S + 1, np.uint32), ctypes.c_int64(-1))
        cnt = np.zeros(1, dtype=np.uint32)
        pc.check(L.shp_dsegpoints_merge_dev(pc.handle, None, 0, 1, _lib.ptr(cnt), 0, S + 1, _lib.ptr(merged),
                                            ctypes.byref(nm)))
        assert nm.value == 0
        (_ids, wx, wy, wv) = C.visit_points(seg, band, 0, tile, S, row0=row0, img_rows=R)
        assert wy.tolist() == [2 ** 31 - 1, 2 ** 31, 2 ** 31 - 1, 2 ** 31] and wv.tolist() == [5, 8, 6, 7]
        offs = np.full(S + 2, -7, dtype=np.int64)
        out = np.zeros(4, dtype=[('x', np.uint32), ('y', np.uint32), ('val', np.int64)])
        n = ctypes.c_int64(-1)
        pc.check(L.shp_dsegpoints_emit(pc.handle, 0, S + 1, _lib.ptr(offs), _lib.ptr(out), 4, ctypes.byref(n)))
        assert n.value == 4 and offs.tolist() == [0, 0, 2, 4]
        assert np.array_equal(out['x'], wx) and np.array_equal(out['y'], wy) and np.array_equal(out['val'], wv)
    finally:
        for p in bufs:
            L.shp_dev_free(cc.handle, p)
        pc.close()
        cc.close()
