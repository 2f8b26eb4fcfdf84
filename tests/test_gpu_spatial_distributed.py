"""GPU: the spatial per-segment statistics split by rows over the ranks
(distributed.calcPerSegmentSpatialStatsDistributed / deviceSpatialStats): on every rank, every column equals
tilingstats.calcPerSegmentSpatialStats of the whole raster bit for bit, and the oracle as
test_spatial_stats_vs_oracle_large compares them."""
import os

import numpy as np
import pytest

from conftest import ROOT

import dist_cases
import spatial_cases as sc
import spatial_dist_helpers as H

pytestmark = pytest.mark.gpu

ROT = [300000.5, 10.25, 0.75, 7000000.25, -0.5, -10.125]       # a rotated, non-integer geotransform


def _cases():
    from pyshepseg_amd import tilingstats as ts
    R, I = ts.GFT_Real, ts.GFT_Integer
    return [('meancoord', ts.userFuncMeanCoord, [300000.0, 10.0, 0.0, 7000000.0, 0.0, -10.0], [R, R], True),
            ('meancoord', ts.userFuncMeanCoord, ROT, [R, R], False),
            ('numedge', ts.userFuncNumEdgePixels, True, [I, I], True),        # second int column stays missing
            ('numedge', ts.userFuncNumEdgePixels, False, [I], True),
            ('variogram', ts.userFuncVariogram, 1, [R], True),
            ('variogram', ts.userFuncVariogram, 5, [R] * 5, True),
            ('variogram', ts.userFuncVariogram, 12, [R] * 13, True)]         # 12 > a 2-row shard; one column more


# row shards: a 2-row shard, an empty shard ((0, 0): a rank without tiles) and segments crossing every boundary
SHARDS = {1: [(0, 61)], 2: [(0, 29), (29, 61)], 3: [(0, 25), (25, 27), (27, 61)],
          4: [(0, 18), (18, 20), (0, 0), (20, 61)]}


@pytest.mark.parametrize('world,dtype,nullv', [(1, np.uint16, 65535), (2, np.uint8, 0), (3, np.int16, -7),
                                               (4, np.uint32, 4000), (4, np.uint16, 3)])
def test_spatial_split_matches_one_gpu(world, dtype, nullv, oracle):
    _check_split(world, dtype, nullv, None, oracle)


@pytest.mark.parametrize('world,dtype,nullv,span', [(2, np.int32, -2 ** 31, 'full'), (3, np.uint32, 2 ** 32 - 1, 'mid'),
                                                    (4, np.int32, 7, 'mid'), (4, np.uint32, 0, 'full')])
def test_spatial_split_wide_values(world, dtype, nullv, span, oracle):
    """32-bit values whose squared differences pass 2^53 (mid) or wrap the reference's int64 square (full): the
    flagged variogram pairs, straddlers among them, are recomputed rank after rank"""
    _check_split(world, dtype, nullv, span, oracle)


@pytest.mark.parametrize('world', [2, 3, 4])
def test_spatial_split_chain_across_shards(world, oracle):
    """spatial_cases' order-sensitive chain (+2^62, small terms lost under its ulp, then about -2^62) down rows
    5..47, across every shard boundary: only the ranks' recomputes carried on in row order give the reference's
    value"""
    _check_split(world, np.uint32, 4000, 'chain', oracle)


def _check_split(world, dtype, nullv, span, oracle):
    from pyshepseg_amd import distributed, tilingstats as ts, _lib
    rng = np.random.default_rng(world * 100 + np.dtype(dtype).itemsize)
    (nr, nc) = (61, 83)
    (seg, band, S) = H.blockRaster(rng, nr, nc, dtype, nullv)
    if span == 'chain':
        sc.plant_chain(seg, band, 5, 20, int(seg.max()) + 1)
        S = int(seg.max()) + 3
    elif span is not None:          # the same nodata pixels, values over the span
        info = np.iinfo(dtype)
        (lo, hi) = (int(info.min), int(info.max)) if span == 'full' else (max(int(info.min), -10 ** 9), 10 ** 9)
        wide = rng.integers(lo, hi, size=band.shape, endpoint=True, dtype=np.int64)
        wide[wide == nullv] = nullv + 1 if nullv < hi else nullv - 1
        band = np.where(band == nullv, nullv, wide).astype(dtype)
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
    hist[0] = 0
    cases = _cases()
    ranges = SHARDS[world]

    def work(c, comm, d_seg, d_band, rr):
        out = []
        for (_name, fn, prm, types, _exact) in cases:
            info = {}
            res = distributed.deviceSpatialStats(c, comm, d_seg, d_band, _lib.SHP_DTYPES[np.dtype(dtype)], nr, nc, rr,
                                                 hist, types, fn, prm, -9999, nullv, info=info)
            out.append(res + (info.get('varioRecomputed'),))
        return out
    (results, errors) = H.runShards(seg, band, ranges, work)
    assert not any(errors), errors
    held = [set(np.unique(seg[a:b])) - {0} for (a, b) in ranges]
    strad = set()
    for i in range(world):
        for j in range(i + 1, world):
            strad |= held[i] & held[j]
    assert world == 1 or len(strad) > 10
    for (k, (name, fn, prm, types, exact)) in enumerate(cases):
        (wi, wf) = ts.calcPerSegmentSpatialStats(seg, band, types, fn, prm, nullv, maxSegId=S)
        oneRedo = ts.variogramRecomputed() if name == 'variogram' else None
        nInt = sum(1 for t in types if t == ts.GFT_Integer)
        (oi, of) = oracle.spatialstats(seg, band, name, prm, nullv, nInt, len(types) - nInt, max_seg_id=S)
        for r in range(world):
            (ic, fc, nStrad, halo, nRedo) = results[r][k]
            assert nStrad == len(strad), (name, prm, r)
            if name == 'variogram':
                assert nRedo == oneRedo, (prm, r)
                assert (nRedo > 0) == (span is not None), (prm, r)
            assert np.array_equal(ic, wi), (name, prm, r)
            assert np.array_equal(fc.view(np.uint32), wf.view(np.uint32)), (name, prm, r)
            assert np.array_equal(ic, oi), (name, prm, r)
            if exact:
                assert np.array_equal(fc.view(np.uint32), of.view(np.uint32)), (name, prm, r)
            else:   # float64 sums of transformed coordinates, re-associated (LABNOTES: 1e-6 relative)
                assert np.allclose(fc, of, rtol=1e-6, atol=0), (name, prm, r)
        assert (wf[:, 5] == -9999).all() and (wi[:, 5] == -9999).all()       # the all-nodata segment
        assert (wf[:, S] == -9999).all() and (wi[:, S] == -9999).all()       # an id nobody holds


@pytest.mark.parametrize('straddler', [False, True])
def test_spatial_split_smallest_exchange(straddler):
    """Two ranks of two rows of a 4 x 3 raster whose labels are constant within a rank's rows: no rank has a record
    to send, so nothing is gathered (the shards above reach that at world 1 only; their empty shard is the rank
    without records beside ranks that have some).  With ``straddler`` one more segment runs down column 0 across
    the boundary."""
    from pyshepseg_amd import distributed, tilingstats as ts
    seg = np.repeat(np.array([1, 1, 2, 2], dtype=np.uint32), 3).reshape(4, 3)
    if straddler:
        seg[1:3, 0] = 3
    band = (np.arange(12, dtype=np.uint16) * 7 + 1).reshape(4, 3)
    hist = np.bincount(seg.ravel(), minlength=4).astype(np.uint32)
    cases = _cases()

    def work(c, comm, d_seg, d_band, rr):
        return [distributed.deviceSpatialStats(c, comm, d_seg, d_band, 2, 4, 3, rr, hist, types, fn, prm, -9999, 0)
                for (_name, fn, prm, types, _exact) in cases]
    (results, errors) = H.runShards(seg, band, [(0, 2), (2, 4)], work, timeout=120)
    assert not any(errors), errors
    for (k, (name, fn, prm, types, _exact)) in enumerate(cases):
        (wi, wf) = ts.calcPerSegmentSpatialStats(seg, band, types, fn, prm, 0, maxSegId=3)
        for r in range(2):
            (ic, fc, nStrad, _halo) = results[r][k]
            assert nStrad == int(straddler), (name, prm, r)
            assert np.array_equal(ic, wi), (name, prm, r)
            assert np.array_equal(fc.view(np.uint32), wf.view(np.uint32)), (name, prm, r)


def test_spatial_split_wrong_histogram_raises_everywhere():
    """a histogram that does not match the labels, too small for one id or too large for another, and a nodata
    value missing on one rank: every rank raises the same error, none hangs in a collective"""
    from pyshepseg_amd import distributed, tilingstats as ts, _lib
    rng = np.random.default_rng(5)
    (nr, nc) = (40, 50)
    (seg, band, S) = H.blockRaster(rng, nr, nc, np.uint16, 9)
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
    hist[0] = 0
    ranges = [(0, 13), (13, 14), (14, 40)]
    low, high = hist.copy(), hist.copy()
    sid = int(seg[0, 0]) if seg[0, 0] else int(seg[0, 1])
    low[sid] -= 1
    high[S] = 7                                      # pixels of an id nobody holds

    for (h, nulls, what) in ((low, [9, 9, 9], 'does not match'), (high, [9, 9, 9], 'does not match'),
                             (hist, [9, None, 9], 'NoData value must be set')):
        def work(c, comm, d_seg, d_band, rr):
            return distributed.deviceSpatialStats(c, comm, d_seg, d_band, 2, nr, nc, rr, h, [ts.GFT_Integer],
                                                  ts.userFuncNumEdgePixels, True, -9999, nulls[comm.rank])
        (results, errors) = H.runShards(seg, band, ranges, work, timeout=120)
        for e in errors:
            assert isinstance(e, ts.PyShepSegStatsError) and what in str(e), errors


def test_spatial_split_refuses_shared_rows():
    """tile-sharded output rows (the ranks share rows, zeros where the other rank writes): edges and the
    variogram are refused on every rank; mean coordinates need no halo and stay exact"""
    from pyshepseg_amd import distributed, tilingstats as ts, _lib
    rng = np.random.default_rng(8)
    (nr, nc) = (30, 40)
    (seg, band, S) = H.blockRaster(rng, nr, nc, np.uint16, 9)
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
    hist[0] = 0
    # two ranks over rows 0..30 and 20..30: rank 1 writes the right part of rows 20..30, rank 0 the rest
    s0, s1 = seg.copy(), seg.copy()
    s0[20:, 25:] = 0
    s1[20:, :25] = 0
    shards = [s0[0:30], s1[20:30]]

    for (fn, prm, types) in ((ts.userFuncNumEdgePixels, False, [ts.GFT_Integer]),
                             (ts.userFuncVariogram, 3, [ts.GFT_Real] * 3),
                             (ts.userFuncMeanCoord, [1.0, 2.0, 0.0, 5.0, 0.0, -3.0], [ts.GFT_Real] * 2)):
        def work(c, comm, d_seg, d_band, rr):
            import ctypes
            lab = np.ascontiguousarray(shards[comm.rank])
            c.check(c._L.shp_dev_upload(c.handle, ctypes.c_void_p(d_seg), _lib.ptr(lab), lab.nbytes))
            return distributed.deviceSpatialStats(c, comm, d_seg, d_band, 2, nr, nc, rr, hist, types, fn, prm,
                                                  -9999, 9)
        (results, errors) = H.runShards(seg, band, [(0, 30), (20, 30)], work, timeout=120)
        if fn is ts.userFuncMeanCoord:
            assert not any(errors), errors
            (wi, wf) = ts.calcPerSegmentSpatialStats(seg, band, types, fn, prm, 9, maxSegId=S)
            for res in results:
                assert np.array_equal(res[1].view(np.uint32), wf.view(np.uint32))
        else:
            for e in errors:
                assert isinstance(e, ts.PyShepSegStatsError) and 'SHEPSEG_SHARD=rows' in str(e), errors


def test_spatial_split_socket_ranks_match_single_process(tmp_path, oracle):
    """runDistributed with the HIP engine, two ranks sharing GPU 0 over sockets (device buffers staged through
    the host), then calcPerSegmentSpatialStatsDistributed == the single-process tiled run + the one-GPU spatial
    statistics of its raster"""
    from pyshepseg_amd import tiling, tilingstats as ts
    import dist_worker_spatial_gpu as W
    (nr, nc, tile, ov, bandnum) = (700, 600, 256, 64, 2)
    band = oracle.synthimg(11, 4, nr, nc)[bandnum - 1]
    nullv = int(np.median(band))
    assert (band == nullv).any()
    dist_cases.runRanks(2, [os.path.join(ROOT, 'tests', 'dist_worker_spatial_gpu.py'), str(tmp_path), str(nr),
                            str(nc), str(tile), str(ov), str(bandnum), str(nullv)], tmp_path, 600)
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
    for (name, fn, prm, cols) in W.CASES:
        types = [ts.GFT_Real if t == 'R' else ts.GFT_Integer for t in cols]
        (wi, wf) = ts.calcPerSegmentSpatialStats(ref.segimg, band, types, getattr(ts, fn), prm, nullv,
                                                 maxSegId=ref.maxSegId)
        for q in parts:
            assert int(q['maxSegId']) == ref.maxSegId
            assert np.array_equal(q[name + '_ic'], wi), name
            assert np.array_equal(q[name + '_fc'].view(np.uint32), wf.view(np.uint32)), name
            assert int(q[name + '_straddlers']) > 0
        assert int(parts[0][name + '_halo']) == {'mean': 0, 'meanrot': 0, 'edge4': 2, 'edge8': 2, 'vario5': 5}[name]


def test_spatial_split_rccl_world_one(tmp_path):
    """the RCCL communicator at world size 1 (a fresh process) carries the whole path: the result equals the
    one-GPU spatial statistics"""
    from pyshepseg_amd import tilingstats as ts  # noqa: F401  (the library builds before the rank starts)
    rng = np.random.default_rng(3)
    (seg, band, S) = H.blockRaster(rng, 57, 70, np.int16, -1)
    np.save(tmp_path / 'seg.npy', seg)
    np.save(tmp_path / 'band.npy', band)
    code = (
        "import sys, ctypes, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from pyshepseg_amd import comm as C, distributed, tilingstats as ts, _lib\n"
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
        "for (fn, prm, types) in ((ts.userFuncMeanCoord, [5.0, 1.0, 0.0, 9.0, 0.0, -1.0], [R, R]),\n"
        "                         (ts.userFuncNumEdgePixels, False, [I]), (ts.userFuncVariogram, 4, [R] * 4)):\n"
        "    info = {}\n"
        "    ic, fc, ns, halo = distributed.deviceSpatialStats(c, comm, ptrs[0].value, ptrs[1].value, 1, seg.shape[0],\n"
        "                                                     seg.shape[1], (0, seg.shape[0]), hist, types, fn, prm, -9999, -1)\n"
        "    wi, wf = ts.calcPerSegmentSpatialStats(seg, band, types, fn, prm, -1, maxSegId=S)\n"
        "    assert np.array_equal(ic, wi) and np.array_equal(fc.view(np.uint32), wf.view(np.uint32)), fn.__name__\n"
        "    assert ns == 0 and halo == 0\n"
        "for p in ptrs:\n"
        "    c.check(c._L.shp_dev_free(c.handle, p))\n"
        "comm.close()\n" % (ROOT, str(tmp_path / 'seg.npy'), str(tmp_path / 'band.npy'), S))
    dist_cases.runRanks(1, ['-c', code], tmp_path, 300)
