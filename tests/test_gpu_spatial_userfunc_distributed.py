"""GPU: user-defined spatial statistics on the row-sharded label raster (distributed.deviceSpatialStats /
calcPerSegmentSpatialStatsDistributed with a spatialUserFunc): every rank's columns equal
tilingstats.calcPerSegmentSpatialStats of the whole raster bit for bit, the user function is called once per id
with points -- by the rank that holds the whole segment, or by the owner of the id's share for a segment that
crosses ranks -- and gets the points in the whole raster's visit order."""
import os

import numpy as np
import pytest

from conftest import ROOT

import dist_cases
import segpoints_helpers as P
import spatial_dist_helpers as H
import spatial_userfunc_dist_helpers as U

pytestmark = pytest.mark.gpu

# row shards as in test_gpu_spatial_distributed.py: a 2-row shard, an empty shard ((0, 0)), segments crossing every
# boundary; none of the boundaries falls on a row of 16- or 7-row tiles
SHARDS = {1: [(0, 61)], 2: [(0, 29), (29, 61)], 3: [(0, 25), (25, 27), (27, 61)],
          4: [(0, 18), (18, 20), (0, 0), (20, 61)]}
(NR, NC) = (61, 83)


def _types():
    from pyshepseg_amd import tilingstats as ts
    return [ts.GFT_Integer, ts.GFT_Real, ts.GFT_Integer, ts.GFT_Real]


def _want(seg, band, nullv, tile, S, prm):
    """(one-GPU columns, numpy restatement of the visit order fed to the same function)"""
    from pyshepseg_amd import tilingstats as ts
    fn = ts.spatialUserFunc(U.order_hash)
    one = ts.calcPerSegmentSpatialStats(seg, band, _types(), fn, prm, nullv, maxSegId=S, tileSize=tile)
    nump = ts.runUserFunc(P.numpy_batches(seg, band, nullv, tile, [(1, S + 1)], S), S + 1, fn, prm, nullv, 2, 2)
    return one, nump


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize('world,dtype,nullv,tile', [(1, np.uint16, 65535, 16), (2, np.uint8, 0, 7),
                                                    (2, np.int32, -5, 64), (3, np.int16, -7, 16),
                                                    (4, np.uint32, 4000, 7), (4, np.uint16, 3, 64)])
def test_userfunc_split_matches_one_gpu(world, dtype, nullv, tile):
    from pyshepseg_amd import distributed, _lib
    rng = np.random.default_rng(world * 1000 + np.dtype(dtype).itemsize * 10 + tile)
    (seg, band, S) = H.blockRaster(rng, NR, NC, dtype, nullv)
    streak = int(np.bincount(seg[:, 3]).argmax())       # a segment down the whole raster, all nodata: a straddler
    band[seg == streak] = nullv                         # without points
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
    hist[0] = 0
    ranges = SHARDS[world]
    calls = [[] for _r in range(world)]
    BATCH = 40                       # the vertical streaks (straddlers of ~55 points) come alone in a batch

    def work(c, comm, d_seg, d_band, rr):
        info = {}
        fn = U.recording(U.order_hash, seg, calls[comm.rank])
        res = distributed.deviceSpatialStats(c, comm, d_seg, d_band, _lib.SHP_DTYPES[np.dtype(dtype)], NR, NC, rr,
                                             hist, _types(), fn, 9, -9999, nullv, tileSize=tile, batchPoints=BATCH,
                                             info=info)
        return res, info
    (results, errors) = H.runShards(seg, band, ranges, work)
    assert not any(errors), errors
    (one, nump) = _want(seg, band, nullv, tile, S, 9)
    assert _same(one, nump)
    for r in range(world):
        (ic, fc, _ns, halo) = results[r][0]
        assert halo == 0
        assert _same((ic, fc), one), r
    # every id with points is called exactly once, by the rank that holds it whole or the owner of its share
    valid = (seg != 0) & (band != nullv)
    withPts = set(np.unique(seg[valid]).tolist())
    allCalls = sum(calls, [])
    assert sorted(allCalls) == sorted(withPts)
    held = [set(np.unique(seg[a:b])) - {0} for (a, b) in ranges]
    strad = set()
    for i in range(world):
        for j in range(i + 1, world):
            strad |= held[i] & held[j]
    assert world == 1 or len(strad) > 10
    for r in range(world):
        (lo, hi) = distributed.idRange(r, world, S)
        want = sorted(i for i in withPts if (i in strad and lo <= i < hi) or (i not in strad and i in held[r]))
        assert calls[r] == want, r                         # ascending id order on each rank
        info = results[r][1]
        assert info['path'] == 'points' and info['calls'] == len(want)
        assert info['straddlers'] == len(strad)
        stradPts = int(np.isin(seg[valid], list(strad)).sum()) if strad else 0
        assert info['points_exchanged'] == stradPts
    # ids without points -- the all-nodata straddler, ids nobody holds -- are missing, row 0 is zero
    noPts = [i for i in range(1, S + 1) if i not in withPts]
    assert streak in noPts and S in noPts and hist[streak] > 0 and hist[S] == 0
    for i in noPts:
        assert (one[0][:, i] == -9999).all() and (one[1][:, i] == -9999).all(), i
    assert (one[0][:, 0] == 0).all() and (one[1][:, 0] == 0).all()


@pytest.mark.parametrize('straddler', [False, True])
def test_userfunc_split_smallest_exchange(straddler):
    """Two ranks of two rows of a 4 x 3 raster whose labels are constant within a rank's rows: no rank has a point
    record to send, so nothing is gathered (the shards above reach that at world 1 only; their empty shard is the
    rank without records beside ranks that have some).  With ``straddler`` one more segment runs down column 0
    across the boundary: its two points travel."""
    from pyshepseg_amd import distributed, tilingstats as ts
    seg = np.repeat(np.array([1, 1, 2, 2], dtype=np.uint32), 3).reshape(4, 3)
    if straddler:
        seg[1:3, 0] = 3
    band = (np.arange(12, dtype=np.uint16) * 7 + 1).reshape(4, 3)
    hist = np.bincount(seg.ravel(), minlength=4).astype(np.uint32)
    fn = ts.spatialUserFunc(U.order_hash)

    def work(c, comm, d_seg, d_band, rr):
        info = {}
        res = distributed.deviceSpatialStats(c, comm, d_seg, d_band, 2, 4, 3, rr, hist, _types(), fn, 9, -9999, 0,
                                             tileSize=2, batchPoints=25, info=info)
        return res, info
    (results, errors) = H.runShards(seg, band, [(0, 2), (2, 4)], work, timeout=120)
    assert not any(errors), errors
    (one, nump) = _want(seg, band, 0, 2, 3, 9)
    assert _same(one, nump)
    for (res, info) in results:
        assert _same(res[:2], one)
        assert info['straddlers'] == int(straddler) and info['points_exchanged'] == 2 * int(straddler)


def test_userfunc_shared_rows_match_one_gpu():
    """tile-sharded output rows (two ranks share rows 20..30, each holding the labels of its part, zeros elsewhere):
    no halo is needed, the points of a segment on both sides interleave by visit index"""
    from pyshepseg_amd import distributed, tilingstats as ts, _lib
    import ctypes
    rng = np.random.default_rng(8)
    (nr, nc) = (30, 40)
    (seg, band, S) = H.blockRaster(rng, nr, nc, np.uint16, 9)
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
    hist[0] = 0
    s0, s1 = seg.copy(), seg.copy()
    s0[20:, 25:] = 0
    s1[20:, :25] = 0
    shards = [s0[0:30], s1[20:30]]
    fn = ts.spatialUserFunc(U.order_hash)
    for tile in (7, 16):
        def work(c, comm, d_seg, d_band, rr):
            lab = np.ascontiguousarray(shards[comm.rank])
            c.check(c._L.shp_dev_upload(c.handle, ctypes.c_void_p(d_seg), _lib.ptr(lab), lab.nbytes))
            return distributed.deviceSpatialStats(c, comm, d_seg, d_band, 2, nr, nc, rr, hist, _types(), fn, 1,
                                                  -9999, 9, tileSize=tile, batchPoints=25)
        (results, errors) = H.runShards(seg, band, [(0, 30), (20, 30)], work, timeout=120)
        assert not any(errors), errors
        (one, nump) = _want(seg, band, 9, tile, S, 1)
        assert _same(one, nump)
        for res in results:
            assert _same(res[:2], one), tile


def test_userfunc_split_errors_raise_everywhere():
    """a user function that raises on a segment rank 1 calls, an undecorated callable and a wrong histogram:
    every rank raises, none hangs in a collective; rank 1 re-raises its own exception"""
    from pyshepseg_amd import distributed, tilingstats as ts
    rng = np.random.default_rng(5)
    (nr, nc) = (40, 50)
    (seg, band, S) = H.blockRaster(rng, nr, nc, np.uint16, 9)
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
    hist[0] = 0
    ranges = [(0, 13), (13, 27), (27, 40)]
    only1 = (set(np.unique(seg[13:27])) - set(np.unique(seg[:13])) - set(np.unique(seg[27:])) - {0})
    valid = (seg != 0) & (band != 9)
    victim = min(i for i in only1 if (valid & (seg == i)).any())

    class Boom(Exception):
        pass

    def bad(pts, nullv, intArr, floatArr, prm):
        if seg[int(pts.y[0]), int(pts.x[0])] == victim:
            raise Boom('segment %d' % victim)
        U.order_hash(pts, nullv, intArr, floatArr, prm)
    low = hist.copy()
    low[victim] -= 1
    for (fn, h, check) in (
            (ts.spatialUserFunc(bad), hist,
             lambda r, e: isinstance(e, Boom) if r == 1 else
             (isinstance(e, ts.PyShepSegStatsError) and 'rank 1' in str(e) and 'Boom' in str(e))),
            (lambda *a: U.order_hash(*a), hist,          # (undecorated)
             lambda r, e: isinstance(e, ts.PyShepSegStatsError) and 'spatialUserFunc' in str(e)),
            (ts.spatialUserFunc(U.order_hash), low,
             lambda r, e: isinstance(e, ts.PyShepSegStatsError) and 'does not match' in str(e))):
        def work(c, comm, d_seg, d_band, rr):
            return distributed.deviceSpatialStats(c, comm, d_seg, d_band, 2, nr, nc, rr, h, _types(), fn, 0,
                                                  -9999, 9, tileSize=16)
        (results, errors) = H.runShards(seg, band, ranges, work, timeout=120)
        for (r, e) in enumerate(errors):
            assert check(r, e), (r, errors)


def test_userfunc_socket_ranks_match_single_process(tmp_path):
    """runDistributed with the HIP engine, two ranks sharing GPU 0 over sockets, then
    calcPerSegmentSpatialStatsDistributed with a user function == the single-process tiled run + the one-GPU
    user-function statistics of its raster"""
    from pyshepseg_amd import tiling, tilingstats as ts
    import dist_worker_spatial_userfunc_gpu as W
    (nr, nc, tile, ov, bandnum) = (700, 600, 256, 64, 2)
    from oracle import oracle as orc
    orc.build()
    band = orc.synthimg(11, 4, nr, nc)[bandnum - 1]
    nullv = int(np.median(band))
    assert (band == nullv).any()
    dist_cases.runRanks(2, [os.path.join(ROOT, 'tests', 'dist_worker_spatial_userfunc_gpu.py'), str(tmp_path),
                            str(nr), str(nc), str(tile), str(ov), str(bandnum), str(nullv)], tmp_path, 600)
    ras = tiling.DeviceRaster.synth(11, 4, nr, nc)
    try:
        cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=2)
        ref = tiling.doTiledShepherdSegmentation(ras, None, tileSize=tile, overlapSize=ov, minSegmentSize=30,
                                                 numClusters=20, fixedKMeansInit=True, concurrencyCfg=cfg)
    finally:
        ras.free()
    parts = [np.load(tmp_path / ('stats%d.npz' % r)) for r in range(2)]
    rows = [(int(q['outLo']), int(q['outHi'])) for q in parts]
    assert rows[0][0] == 0 and rows[0][1] == rows[1][0] and rows[1][1] == nr and 0 < rows[1][0] < nr
    fn = ts.spatialUserFunc(U.order_hash)
    valid = (ref.segimg != 0) & (band != nullv)
    for ts_ in W.TILES:
        (wi, wf) = ts.calcPerSegmentSpatialStats(ref.segimg, band, W._types(), fn, W.PARAM, nullv,
                                                 maxSegId=ref.maxSegId, tileSize=ts_)
        for q in parts:
            assert int(q['maxSegId']) == ref.maxSegId
            assert np.array_equal(q['ic%d' % ts_], wi), ts_
            assert np.array_equal(q['fc%d' % ts_].view(np.uint32), wf.view(np.uint32)), ts_
            assert int(q['straddlers%d' % ts_]) > 0
        assert sum(int(q['calls%d' % ts_]) for q in parts) == len(np.unique(ref.segimg[valid]))


def test_userfunc_rccl_world_one(tmp_path):
    """the RCCL communicator at world size 1 (a fresh process) carries the user-function path: the result equals
    the one-GPU user-function statistics"""
    from pyshepseg_amd import tilingstats as ts  # noqa: F401  (the library builds before the rank starts)
    rng = np.random.default_rng(3)
    (seg, band, S) = H.blockRaster(rng, 57, 70, np.int16, -1)
    np.save(tmp_path / 'seg.npy', seg)
    np.save(tmp_path / 'band.npy', band)
    code = (
        "import sys, ctypes, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from pyshepseg_amd import comm as C, distributed, tilingstats as ts, _lib\n"
        "import spatial_userfunc_dist_helpers as U\n"
        "comm = C.RcclComm()\n"
        "assert (comm.rank, comm.world) == (0, 1) and comm.onDevice\n"
        "seg = np.load(%r); band = np.load(%r); S = %d\n"
        "hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32); hist[0] = 0\n"
        "c = _lib.ctx()\n"
        "ptrs = []\n"
        "for a in (seg, band):\n"
        "    p = ctypes.c_void_p(); c.check(c._L.shp_dev_alloc(c.handle, a.nbytes, ctypes.byref(p)))\n"
        "    c.check(c._L.shp_dev_upload(c.handle, p, _lib.ptr(a), a.nbytes)); ptrs.append(p)\n"
        "R, I = ts.GFT_Real, ts.GFT_Integer\n"
        "fn = ts.spatialUserFunc(U.order_hash)\n"
        "for tile in (16, 1024):\n"
        "    info = {}\n"
        "    ic, fc, ns, halo = distributed.deviceSpatialStats(c, comm, ptrs[0].value, ptrs[1].value, 1, seg.shape[0],\n"
        "        seg.shape[1], (0, seg.shape[0]), hist, [I, R, I], fn, 3, -9999, -1, tileSize=tile, info=info)\n"
        "    wi, wf = ts.calcPerSegmentSpatialStats(seg, band, [I, R, I], fn, 3, -1, maxSegId=S, tileSize=tile)\n"
        "    assert np.array_equal(ic, wi) and np.array_equal(fc.view(np.uint32), wf.view(np.uint32)), tile\n"
        "    assert ns == 0 and halo == 0 and info['path'] == 'points' and info['points_exchanged'] == 0\n"
        "for p in ptrs:\n"
        "    c.check(c._L.shp_dev_free(c.handle, p))\n"
        "comm.close()\n" % (ROOT, os.path.join(ROOT, 'tests'), str(tmp_path / 'seg.npy'), str(tmp_path / 'band.npy'),
                            S))
    dist_cases.runRanks(1, ['-c', code], tmp_path, 300)


def test_dsegpoints_entry_points_order():
    """shp_dsegpoints_merge_dev and _emit refuse to run out of order"""
    import ctypes
    from pyshepseg_amd import _lib
    c = _lib.Context()
    try:
        L = c._L
        offs = np.zeros(4, np.int64)
        (n, cnt) = (ctypes.c_int64(0), np.zeros(1, np.uint32))
        with pytest.raises(_lib.ShepsegHipError, match='shp_dsegpoints_build_dev'):
            c.check(L.shp_dsegpoints_merge_dev(c.handle, None, 0, 1, _lib.ptr(cnt), 0, 3, _lib.ptr(offs),
                                               ctypes.byref(n)))
        with pytest.raises(_lib.ShepsegHipError, match='shp_dsegpoints_merge_dev'):
            c.check(L.shp_dsegpoints_emit(c.handle, 0, 3, _lib.ptr(offs), None, 0, ctypes.byref(n)))
    finally:
        c.close()
