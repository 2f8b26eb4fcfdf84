"""GPU: subset.subsetImage on the row-sharded label raster (distributed.deviceSubset / subsetImageDistributed):
every rank's origSegIds, hist and columns equal subset.subsetImage of the whole raster bit for bit, and the ranks'
recoded rows, stacked by their window rows, equal its segimg."""
import os

import numpy as np
import pytest

from conftest import ROOT

import dist_cases
import spatial_dist_helpers as H

pytestmark = pytest.mark.gpu

# row shards as in the spatial tests: a 2-row shard, an empty shard ((0, 0)); no boundary falls on a row of 16- or
# 7-row tiles of a window from row 0
SHARDS = {1: [(0, 61)], 2: [(0, 29), (29, 61)], 3: [(0, 25), (25, 27), (27, 61)],
          4: [(0, 18), (18, 20), (0, 0), (20, 61)]}
(NR, NC) = (61, 83)


def _holes(ys, xs):
    rng = np.random.default_rng(ys * 1000 + xs)
    m = (rng.random((ys, xs)) > 0.25).astype(np.uint8)
    m[ys // 3:ys // 3 + 6, xs // 4:xs // 4 + 9] = 0
    return m


# (tlx, tly, xs, ys, mask): the whole raster, inside one shard (rows 33..53 of every layout's last shard), across
# every boundary, at the image's bottom-right border, with a mask with holes
WINDOWS = [(0, 0, NC, NR, None), (5, 33, 60, 20, None), (3, 2, 77, 57, None), (50, 40, 33, 21, None),
           (0, 10, NC, 45, _holes(45, NC))]


class _ShardEngine(object):
    """the HipEngine side subsetImageDistributed uses, over one thread-rank's rows"""
    def __init__(self, c, d_seg, rr, nCols=NC):
        (self.c, self.d_seg, self.rr, self.nCols) = (c, d_seg, rr, nCols)

    def subsetOnDevice(self, comm, maxSegId, tlx, tly, xs, ys, mask=None, tileSize=None):
        from pyshepseg_amd import distributed
        return distributed.deviceSubset(self.c, comm, self.d_seg, None, self.nCols, self.rr, maxSegId, tlx, tly, xs,
                                        ys, mask=mask, tileSize=tileSize)


class _Result(object):
    def __init__(self, maxSegId):
        self.maxSegId = maxSegId


def _raster(seed):
    rng = np.random.default_rng(seed)
    (seg, _band, S) = H.blockRaster(rng, NR, NC, np.uint16, 9)
    return seg, S


def _stack(parts, shape):
    out = np.full(shape, 0xFFFFFFFF, dtype=np.uint32)
    for (rows, (a, b)) in parts:
        assert rows.shape == (b - a, shape[1])
        assert (out[a:b] == 0xFFFFFFFF).all()
        out[a:b] = rows
    return out


@pytest.mark.parametrize('world', [1, 2, 3, 4])
@pytest.mark.parametrize('tile', [16, 7, 1024])
def test_subset_split_matches_one_gpu(world, tile, oracle, tmp_path):
    from pyshepseg_amd import distributed, subset
    (seg, S) = _raster(world * 10 + tile)
    col = (np.arange(S + 1, dtype=np.float64) * 1.25 + 3)
    kcol = np.arange(S + 1, dtype=np.int32)[::-1].copy()
    ranges = SHARDS[world]
    out = str(tmp_path / 'sub.npy')

    def work(c, comm, d_seg, _d_band, rr):
        got = []
        for (k, (tlx, tly, xs, ys, m)) in enumerate(WINDOWS):
            info = {}
            low = distributed.deviceSubset(c, comm, d_seg, NR, NC, rr, S, tlx, tly, xs, ys, mask=m, tileSize=tile,
                                           info=info)
            res = distributed.subsetImageDistributed(
                _ShardEngine(c, d_seg, rr), comm, _Result(S), tlx, tly, xs, ys, outname=out if k == 4 else None,
                origSegIdColName='orig', maskImage=m, ratColumns={'v': col, 'k': kcol}, tileSize=tile)
            got.append((low, info, res))
        return got
    (results, errors) = H.runShards(seg, np.zeros(seg.shape, np.uint8), ranges, work)
    assert not any(errors), errors
    for (k, (tlx, tly, xs, ys, m)) in enumerate(WINDOWS):
        want = subset.subsetImage(seg, None, tlx, tly, xs, ys, maskImage=m, tileSize=tile, origSegIdColName='orig',
                                  ratColumns={'v': col, 'k': kcol})
        (wout, worig, whist) = oracle.subset_recode(seg, tlx, tly, xs, ys, m, tile)
        assert np.array_equal(want.segimg, wout) and np.array_equal(want.origSegIds, worig)
        assert np.array_equal(want.hist, whist)
        lows = [results[r][k][0] for r in range(world)]
        win = seg[tly:tly + ys, tlx:tlx + xs] * (1 if m is None else m)
        nPairs = sum(len(set(np.unique(win[a:b]).tolist()) - {0})
                     for (a, b) in (distributed.subsetHeldRows(rr, tly, ys) for rr in ranges))
        ress = [results[r][k][2] for r in range(world)]
        for r in range(world):
            (rows, ab, orig, hist) = lows[r]
            assert ab == distributed.subsetHeldRows(ranges[r], tly, ys)
            assert np.array_equal(orig, want.origSegIds), (k, r)
            assert np.array_equal(hist, want.hist), (k, r)
            q = ress[r]
            assert q.rows == ab and np.array_equal(q.segimg, rows)
            assert np.array_equal(q.origSegIds, want.origSegIds) and np.array_equal(q.hist, want.hist)
            assert list(q.columns) == list(want.columns)
            for name in want.columns:
                assert q.columns[name].dtype == want.columns[name].dtype
                assert np.array_equal(q.columns[name], want.columns[name]), (k, r, name)
            assert results[r][k][1]['pairs'] == nPairs
        assert np.array_equal(_stack([(lw[0], lw[1]) for lw in lows], (ys, xs)), want.segimg), k
        if k == 4:
            assert np.array_equal(np.load(out), want.segimg)


def _expectEveryRank(errors, match):
    from pyshepseg_amd import subset
    for e in errors:
        assert isinstance(e, subset.PyShepSegSubsetError), errors
        assert match in str(e), errors


def test_subset_split_errors_raise_everywhere():
    """an out-of-bounds window, an all-masked window, an id above maxSegId on one rank only and a mask of the
    wrong shape: every rank raises the same error, none is left in a collective"""
    from pyshepseg_amd import distributed
    (seg, S) = _raster(77)
    bad = seg.copy()
    bad[40, 11] = S + 5                           # on rank 2 of SHARDS[3] only
    ranges = SHARDS[3]
    zero = np.zeros((20, 30), np.uint8)
    for (ras, win, mask, match) in ((seg, (0, 50, 10, 12), None, 'not within input image'),
                                    (seg, (60, 0, 24, 5), None, 'not within input image'),
                                    (seg, (5, 10, 30, 20), zero, 'No valid data found in subset'),
                                    (bad, (5, 10, 30, 40), None, 'above maxSegId'),
                                    (seg, (5, 10, 30, 20), np.ones((20, 31), np.uint8), 'mask should match')):
        def work(c, comm, d_seg, _d_band, rr):
            return distributed.deviceSubset(c, comm, d_seg, NR, NC, rr, S, *win, mask=mask, tileSize=7)
        (results, errors) = H.runShards(ras, np.zeros(seg.shape, np.uint8), ranges, work, timeout=120)
        _expectEveryRank(errors, match)
        assert len({str(e) for e in errors}) == 1
    # a window without labels: all null
    hole = seg.copy()
    hole[20:40, 10:50] = 0

    def work(c, comm, d_seg, _d_band, rr):
        return distributed.deviceSubset(c, comm, d_seg, NR, NC, rr, S, 10, 20, 40, 20, tileSize=16)
    (results, errors) = H.runShards(hole, np.zeros(seg.shape, np.uint8), ranges, work, timeout=120)
    _expectEveryRank(errors, 'No valid data found in subset')


def test_subset_split_refuses_shared_rows():
    """tile-sharded output rows (two ranks share rows 20..30) are refused on every rank"""
    from pyshepseg_amd import distributed
    (seg, S) = _raster(5)

    def work(c, comm, d_seg, _d_band, rr):
        return distributed.subsetImageDistributed(_ShardEngine(c, d_seg, rr), comm, _Result(S), 0, 0, NC, NR)
    (results, errors) = H.runShards(seg, np.zeros(seg.shape, np.uint8), [(0, 30), (20, 61)], work, timeout=120)
    _expectEveryRank(errors, 'disjoint output rows')


def test_subset_split_reference_anchor(golden):
    """the CI scenario's mosaic in three row shards that cut the window: the reference's subset goldens"""
    from pyshepseg_amd import distributed
    g = golden('ci_scenario_1000')
    mosaic = g['mosaic']
    S = int(g['max_seg_id'])
    ranges = [(0, 560), (560, 561), (561, 1000)]

    def work(c, comm, d_seg, _d_band, rr):
        eng = _ShardEngine(c, d_seg, rr, mosaic.shape[1])
        return distributed.subsetImageDistributed(eng, comm, _Result(S), 500, 500, 125, 125,
                                                  origSegIdColName='orig_val')
    (results, errors) = H.runShards(mosaic, np.zeros(mosaic.shape, np.uint8), ranges, work, timeout=120)
    assert not any(errors), errors
    assert [q.rows for q in results] == [(0, 60), (60, 61), (61, 125)]
    for q in results:
        assert np.array_equal(q.origSegIds, g['subset_orig']) and np.array_equal(q.hist, g['subset_hist'])
        assert np.array_equal(q.columns['orig_val'], g['subset_orig'].astype(np.int32))
    assert np.array_equal(np.concatenate([q.segimg for q in results]), g['subset_out'])


def test_subset_socket_ranks_match_single_process(tmp_path):
    """runDistributed with the HIP engine, two ranks sharing GPU 0 over sockets, then subsetImageDistributed with a
    mask and a .npy output == subset.subsetImage of the single-process tiled run's raster"""
    from pyshepseg_amd import tiling, subset
    import dist_worker_subset_gpu as W
    (nr, nc, tile, ov) = (700, 600, 256, 64)
    (tlx, tly, xs, ys) = W.WINDOW
    mask = (np.random.default_rng(6).random((ys, xs)) > 0.2).astype(np.uint8)
    np.save(tmp_path / 'mask.npy', mask)
    dist_cases.runRanks(2, [os.path.join(ROOT, 'tests', 'dist_worker_subset_gpu.py'), str(tmp_path), str(nr),
                            str(nc), str(tile), str(ov)], tmp_path, 600)
    ras = tiling.DeviceRaster.synth(11, 4, nr, nc)
    try:
        cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=2)
        ref = tiling.doTiledShepherdSegmentation(ras, None, tileSize=tile, overlapSize=ov, minSegmentSize=30,
                                                 numClusters=20, fixedKMeansInit=True, concurrencyCfg=cfg)
    finally:
        ras.free()
    want = subset.subsetImage(ref.segimg, None, tlx, tly, xs, ys, maskImage=mask, origSegIdColName='orig',
                              ratColumns={'v': W.column(ref.maxSegId)})
    assert np.array_equal(np.load(tmp_path / 'sub.npy'), want.segimg)
    parts = [np.load(tmp_path / ('subset%d.npz' % r)) for r in range(2)]
    outRows = [(int(q['outLo']), int(q['outHi'])) for q in parts]
    assert outRows[0][0] == 0 and outRows[0][1] == outRows[1][0] and tly < outRows[1][0] < tly + ys
    for q in parts:
        assert int(q['maxSegId']) == ref.maxSegId
        (a, b) = (int(q['a']), int(q['b']))
        assert 0 <= a < b <= ys
        assert np.array_equal(q['rows'], want.segimg[a:b])
        assert np.array_equal(q['orig'], want.origSegIds) and np.array_equal(q['hist'], want.hist)
        for name in ('v', 'Histogram', 'orig'):
            assert np.array_equal(q['col_' + name], want.columns[name]), name


def test_subset_rccl_world_one(tmp_path):
    """the RCCL communicator at world size 1 (a fresh process) carries deviceSubset: the result equals
    subset.subsetImage"""
    from pyshepseg_amd import subset  # noqa: F401  (the library builds before the rank starts)
    (seg, S) = _raster(3)
    np.save(tmp_path / 'seg.npy', seg)
    code = (
        "import sys, ctypes, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from pyshepseg_amd import comm as C, distributed, subset, _lib\n"
        "comm = C.RcclComm()\n"
        "assert (comm.rank, comm.world) == (0, 1) and comm.onDevice\n"
        "seg = np.load(%r); S = %d\n"
        "c = _lib.ctx()\n"
        "p = ctypes.c_void_p(); c.check(c._L.shp_dev_alloc(c.handle, seg.nbytes, ctypes.byref(p)))\n"
        "c.check(c._L.shp_dev_upload(c.handle, p, _lib.ptr(seg), seg.nbytes))\n"
        "mask = (np.arange(40 * 50).reshape(40, 50) %% 7 != 0).astype(np.uint8)\n"
        "for (tile, m) in ((16, None), (1024, mask)):\n"
        "    rows, ab, orig, hist = distributed.deviceSubset(c, comm, p.value, None, seg.shape[1], (0, seg.shape[0]),\n"
        "        S, 20, 15, 50, 40, mask=m, tileSize=tile)\n"
        "    w = subset.subsetImage(seg, None, 20, 15, 50, 40, maskImage=m, tileSize=tile)\n"
        "    assert ab == (0, 40) and np.array_equal(rows, w.segimg), tile\n"
        "    assert np.array_equal(orig, w.origSegIds) and np.array_equal(hist, w.hist), tile\n"
        "c.check(c._L.shp_dev_free(c.handle, p))\n"
        "comm.close()\n" % (ROOT, str(tmp_path / 'seg.npy'), S))
    dist_cases.runRanks(1, ['-c', code], tmp_path, 300)
