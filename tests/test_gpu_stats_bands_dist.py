"""GPU: per-segment statistics of one or several bands in ONE call on the row-sharded multi-rank output
(distributed.calcPerSegmentStatsDistributedBands / deviceStatsBands; shp_dstats_local_bands_dev,
shp_dstats_merge_bands_dev).  Every column bit for bit against the one-band distributed call of its entry
(deviceStats, the same driver with one entry) and against the oracle on the whole raster, which is what keeps the
first comparison honest; nothing here has a tolerance."""
import os

import numpy as np
import pytest

from conftest import ROOT

import dist_cases
import stats_bands_dist_helpers as H

pytestmark = pytest.mark.gpu

# three entries over two planes (plane 0 twice), all eight statistics somewhere
ENTRY_PLANES = [0, 1, 0]
ENTRY_SELS = [[('a_min', 'min'), ('a_mean', 'mean'), ('a_med', 'median'), ('a_n', 'pixcount')],
              [('b_max', 'max'), ('b_sd', 'stddev'), ('b_mode', 'mode')],
              [('c_p30', 'percentile', 30), ('c_n', 'pixcount'), ('c_sd', 'stddev'), ('c_min', 'min')]]
NULL_FORMS = {'none': [None, None, None], 'all': [7, 7, 7], 'entry': [7, None, 9]}
DTYPES = [np.uint8, np.int16, np.uint16, np.int32, np.uint32]


def _planes(dtype, seg, nulls, rng):
    info = np.iinfo(dtype)
    planes = [rng.integers(max(info.min, -300), min(info.max, 300) + 1, size=seg.shape).astype(dtype) for _ in range(2)]
    for v in sorted(set(n for n in nulls if n is not None)):
        for p in planes:
            p[rng.random(seg.shape) < 0.08] = v
    if nulls[0] is not None:
        planes[0][seg == _allNullId(seg)] = nulls[0]    # a segment without a valid pixel (for the entries with that null)
    return planes


def _allNullId(seg):
    return int(np.unique(seg[seg != 0])[4])


def _entryColumns(fast, ic, fc, k):
    """entry k's columns out of the combined ones, in the entry's order: [(is int, column)]"""
    from pyshepseg_amd import tilingstats
    first = sum(len(s) for s in ENTRY_SELS[:k])
    cols = []
    for row in fast[first:first + len(ENTRY_SELS[k])]:
        isInt = row[tilingstats.STATSEL_COLTYPE] == tilingstats.STAT_DTYPE_INT
        cols.append((bool(isInt), (ic if isInt else fc)[row[tilingstats.STATSEL_COLARRAYINDEX]]))
    return cols


def _sameBits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
    return a.dtype == b.dtype and np.array_equal(a, b)


def _combined():
    from pyshepseg_amd import tilingstats
    (fast, _bandOfStat, nInt, nFloat) = tilingstats.makeBandStatsSelection(
        [(p + 1, s) for (p, s) in zip(ENTRY_PLANES, ENTRY_SELS)])
    perBand = np.array([len(s) for s in ENTRY_SELS], dtype=np.int32)
    return fast, perBand, nInt, nFloat


def _rankBody(seg, planes, nulls, hist, dtype, world, oneBandToo=True, cuts=None):
    """what every rank thread does: deviceStatsBands on its row shard, then deviceStats per entry.  A rank without
    rows passes made-up band addresses and no pixel type, as HipEngine.statsBandsOnDevice does."""
    import ctypes
    from pyshepseg_amd import distributed, tilingstats, _lib
    (fast, perBand, nInt, nFloat) = _combined()
    cuts = cuts or H.cutsOf(world)
    code = _lib.SHP_DTYPES[np.dtype(dtype)]
    hasNull = [int(v is not None) for v in nulls]
    nullArr = [0 if v is None else int(v) for v in nulls]

    def body(r, comm, c):
        (lo, hi) = (cuts[r], cuts[r + 1])
        ds = H.uploadRows(c, seg[lo:hi])
        dp = [H.uploadRows(c, p[lo:hi]) for p in planes]
        try:
            if hi > lo:
                res = distributed.deviceStatsBands(c, comm, ds.value, [dp[p].value for p in ENTRY_PLANES], code, hi - lo,
                                                   H.NC, hist, fast, perBand, hasNull, nullArr, nInt, nFloat, -9999)
            else:
                res = distributed.deviceStatsBands(c, comm, 0, [16 * (p + 1) for p in ENTRY_PLANES], None, 0, H.NC, hist,
                                                   fast, perBand, hasNull, nullArr, nInt, nFloat, -9999)
            ones = []
            for (k, sel) in enumerate(ENTRY_SELS if oneBandToo else []):
                (f1, n1, m1) = tilingstats.makeFastStatsSelection(list(range(len(sel))), sel)
                ones.append(distributed.deviceStats(c, comm, ds.value, dp[ENTRY_PLANES[k]].value, code, hi - lo, H.NC, hist,
                                                    f1, n1, m1, -9999, nulls[k]))
        finally:
            for d in [ds] + dp:
                c.check(c._L.shp_dev_free(c.handle, d))
        return res, ones
    return body


def _cases():
    return [pytest.param(field, world, dtype, form, patch,
                         id='%s-w%d-%s-%s-patch%d' % (field, world, np.dtype(dtype).name, form, patch))
            for field in 'AB' for world in (2, 3, 4) for dtype in DTYPES for form in NULL_FORMS for patch in (0, 1)]


@pytest.mark.parametrize('field,world,dtype,form,patch', _cases())
def test_device_stats_bands_split(field, world, dtype, form, patch, oracle, monkeypatch):
    """The device path with `world` row shards of one raster on this GPU: three entries over two planes in one
    call == the oracle on the whole raster per entry == deviceStats per entry, on every rank, bit for bit.
    Field A: nearly every segment straddles; field B: most segments are whole on one rank and the last rank's id
    share is nearly empty."""
    monkeypatch.setenv('SHEPSEG_STATS_PATCH', str(patch))
    seed = 1 + (world + DTYPES.index(dtype) + list(NULL_FORMS).index(form)) % 3        # seeds 1-3
    rng = np.random.default_rng(seed)
    (seg, S) = H.labelField(field, rng)
    nulls = NULL_FORMS[form]
    planes = _planes(dtype, seg, nulls, rng)
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
    hist[0] = 0
    # ---- what the case relies on, counted with numpy
    cnt = H.countField(seg, S, world)
    assert len(cnt['strad']) >= 50
    if field == 'A':
        assert min(cnt['perShare']) >= 1, cnt['perShare']
    else:
        assert min(cnt['whole']) >= 100, cnt['whole']
    itemsize = np.dtype(dtype).itemsize
    wantBytes = cnt['pixels'] * (4 + 2 * itemsize)
    assert wantBytes < len(ENTRY_SELS) * (4 + itemsize) * cnt['pixels']      # (three calls with one entry each)
    print('field %s world %d: %d straddlers (%s per id share), %d of %d pixels, whole per rank %s, %d bytes exchanged '
          'against %d of three one-band calls' % (field, world, len(cnt['strad']), cnt['perShare'], cnt['pixels'],
                                                  int((seg != 0).sum()), cnt['whole'], wantBytes,
                                                  3 * (4 + itemsize) * cnt['pixels']))
    (results, errors) = H.runRankThreads(world, _rankBody(seg, planes, nulls, hist, dtype, world))
    assert not any(errors), errors
    (fast, _perBand, nInt, nFloat) = _combined()
    from pyshepseg_amd import tilingstats
    want = [oracle.segstats(seg, planes[ENTRY_PLANES[k]], sel, nulls[k], -9999, max_seg_id=S)
            for (k, sel) in enumerate(ENTRY_SELS)]
    if nulls[0] is not None:                            # the all-null segment is what it is meant to be
        nCol = [s[1] for s in ENTRY_SELS[0]].index('pixcount')
        own = tilingstats.makeFastStatsSelection(list(range(len(ENTRY_SELS[0]))), ENTRY_SELS[0])[0]
        assert int(want[0][0][own[nCol][tilingstats.STATSEL_COLARRAYINDEX]][_allNullId(seg)]) == 0
    for (r, ((ic, fc, nStrad, nPix, nBytes), ones)) in enumerate(results):
        assert ic.shape == (nInt, S + 1) and fc.shape == (nFloat, S + 1)
        assert (nStrad, nPix, nBytes) == (len(cnt['strad']), cnt['pixels'], wantBytes), r
        for (k, sel) in enumerate(ENTRY_SELS):
            own = tilingstats.makeFastStatsSelection(list(range(len(sel))), sel)[0]
            (ic1, fc1, nStrad1, nPix1) = ones[k]
            assert (nStrad1, nPix1) == (nStrad, nPix)
            for ((isInt, col), o, s) in zip(_entryColumns(fast, ic, fc, k), own, sel):
                idx = o[tilingstats.STATSEL_COLARRAYINDEX]
                assert _sameBits(col, (want[k][0] if isInt else want[k][1])[idx]), ('oracle', r, k, s)
                assert _sameBits(col, (ic1 if isInt else fc1)[idx]), ('one band', r, k, s)


@pytest.mark.parametrize('cuts', [[0, 100, 100, 203], [0, 0, 90, 203], [0, 120, 203, 203]])
def test_rank_without_rows_takes_part(cuts, oracle):
    """more ranks than row shards: the rank without rows (the first, a middle one, the last) joins every collective
    with zero pairs, learns the pixel type from the others, reduces its id share, and gets the same columns"""
    from pyshepseg_amd import tilingstats
    rng = np.random.default_rng(2)
    (seg, S) = H.labelField('A', rng)
    nulls = NULL_FORMS['entry']
    planes = _planes(np.int16, seg, nulls, rng)
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
    hist[0] = 0
    (results, errors) = H.runRankThreads(3, _rankBody(seg, planes, nulls, hist, np.int16, 3, oneBandToo=False, cuts=cuts))
    assert not any(errors), errors
    (fast, _perBand, _nInt, _nFloat) = _combined()
    want = [oracle.segstats(seg, planes[ENTRY_PLANES[k]], sel, nulls[k], -9999, max_seg_id=S)
            for (k, sel) in enumerate(ENTRY_SELS)]
    rows = [c for c in zip(cuts[:-1], cuts[1:]) if c[1] > c[0]]
    strad = (set(np.unique(seg[rows[0][0]:rows[0][1]]).tolist()) & set(np.unique(seg[rows[1][0]:rows[1][1]]).tolist())) - {0}
    assert len(strad) >= 50
    for (r, ((ic, fc, nStrad, nPix, nBytes), _ones)) in enumerate(results):
        assert (nStrad, nPix) == (len(strad), int(np.isin(seg, sorted(strad)).sum())) and nBytes == nPix * (4 + 2 * 2)
        for (k, sel) in enumerate(ENTRY_SELS):
            own = tilingstats.makeFastStatsSelection(list(range(len(sel))), sel)[0]
            for ((isInt, col), o, s) in zip(_entryColumns(fast, ic, fc, k), own, sel):
                assert _sameBits(col, (want[k][0] if isInt else want[k][1])[o[tilingstats.STATSEL_COLARRAYINDEX]]), (r, k, s)


@pytest.mark.parametrize('world', [2, 3])
def test_stale_histogram_raises_on_every_rank(world):
    """A histogram that gives one id fewer pixels than a rank holds of it: the library reports it (an argument
    error, counted by a kernel), and every rank raises -- the rank that found it and the ranks that did not --
    and returns."""
    from pyshepseg_amd import _lib
    rng = np.random.default_rng(5)
    (seg, S) = H.labelField('B', rng)
    planes = _planes(np.uint16, seg, NULL_FORMS['none'], rng)
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
    hist[0] = 0
    cnt = H.countField(seg, S, world)
    victim = sorted(cnt['held'][world - 1] - cnt['strad'])[0]          # whole on the last rank
    assert hist[victim] > 1
    hist[victim] -= 1
    (results, errors) = H.runRankThreads(world, _rankBody(seg, planes, NULL_FORMS['none'], hist, np.uint16, world,
                                                          oneBandToo=False), timeout=120)
    assert results == [None] * world
    for (r, e) in enumerate(errors):
        assert isinstance(e, _lib.ShepsegHipError), (r, e)
        assert '1 segment ids have more pixels' in str(e), (r, e)


# ---- one entry: no special route (nbands = nplanes = 1), but the library's one-band statistics kernels
ONE_SEL = [('o_min', 'min'), ('o_max', 'max'), ('o_mean', 'mean'), ('o_sd', 'stddev'), ('o_med', 'median'),
           ('o_mode', 'mode'), ('o_p30', 'percentile', 30), ('o_n', 'pixcount')]


def _widePlane(dtype, seg, null, rng):
    """plane 0 of _planes with a multiple of 2^20 added to a third of the pixels: values that need all four bytes of
    a 4-byte pixel on the wire (null pixels stay null)"""
    plane = _planes(dtype, seg, [null, None, null], rng)[0]
    lift = (rng.integers(1, 4, size=seg.shape) << 20).astype(dtype)
    where = rng.random(seg.shape) < 0.33
    if null is not None:
        where &= plane != null
    plane[where] += lift[where]
    assert int(plane.max()) >= 1 << 20
    return plane


def _oneEntryBody(seg, plane, null, hist, dtype, world, cuts=None, bandsToo=True):
    """what every rank thread does with ONE entry: deviceStatsBands (bandsToo), then deviceStats.  A rank without rows
    passes a made-up band address and no pixel type."""
    from pyshepseg_amd import distributed, tilingstats, _lib
    (f1, n1, m1) = tilingstats.makeFastStatsSelection(list(range(len(ONE_SEL))), ONE_SEL)
    cuts = cuts or H.cutsOf(world)
    code = _lib.SHP_DTYPES[np.dtype(dtype)]

    def body(r, comm, c):
        (lo, hi) = (cuts[r], cuts[r + 1])
        ds = H.uploadRows(c, seg[lo:hi])
        dp = H.uploadRows(c, plane[lo:hi])
        (d_seg, d_band, dt) = (ds.value, dp.value, code) if hi > lo else (0, 16, None)
        try:
            res = None
            if bandsToo:
                res = distributed.deviceStatsBands(c, comm, d_seg, [d_band], dt, hi - lo, H.NC, hist, f1, [len(ONE_SEL)],
                                                   [int(null is not None)], [0 if null is None else null], n1, m1, -9999)
            one = distributed.deviceStats(c, comm, d_seg, d_band, dt, hi - lo, H.NC, hist, f1, n1, m1, -9999, null)
        finally:
            for d in (ds, dp):
                c.check(c._L.shp_dev_free(c.handle, d))
        return res, one
    return body


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('null', [None, 7])
@pytest.mark.parametrize('patch', [0, 1])
@pytest.mark.parametrize('dtype', [np.int32, np.uint32], ids=['int32', 'uint32'])
def test_one_entry_four_byte_pixels(dtype, patch, null, world, oracle, monkeypatch):
    """One entry of a 4-byte pixel type through deviceStatsBands and through deviceStats (its wrapper): every column ==
    the oracle on the whole raster, bit for bit, on every rank; the straddlers' values travel in the pixel type, 4 +
    4 bytes a pixel.  (The library computes one entry with k_stats_patch / the one-band sorts, several with
    k_stats_patch_bands: SHEPSEG_STATS_PATCH 0 and 1 take both forms of the former.)"""
    monkeypatch.setenv('SHEPSEG_STATS_PATCH', str(patch))
    rng = np.random.default_rng(3)
    (seg, S) = H.labelField('A', rng)
    plane = _widePlane(dtype, seg, null, rng)
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
    hist[0] = 0
    cnt = H.countField(seg, S, world)
    assert len(cnt['strad']) >= 50
    (wic, wfc) = oracle.segstats(seg, plane, ONE_SEL, null, -9999, max_seg_id=S)
    if null is not None:
        assert int(wic[-1][_allNullId(seg)]) == 0            # (pixcount, the last integer column)
    (results, errors) = H.runRankThreads(world, _oneEntryBody(seg, plane, null, hist, dtype, world))
    assert not any(errors), errors
    for (r, ((ic, fc, nStrad, nPix, nBytes), (ic1, fc1, nStrad1, nPix1))) in enumerate(results):
        assert (nStrad, nPix, nBytes) == (len(cnt['strad']), cnt['pixels'], cnt['pixels'] * (4 + 4)), r
        assert (nStrad1, nPix1) == (len(cnt['strad']), cnt['pixels']), r
        assert _sameBits(ic, wic) and _sameBits(fc, wfc), ('deviceStatsBands', r)
        assert _sameBits(ic1, wic) and _sameBits(fc1, wfc), ('deviceStats', r)


def test_one_entry_rank_without_rows(oracle):
    """deviceStats with more ranks than row shards: the middle rank passes nRows 0, a made-up band address and no pixel
    type, and gets the same columns as the others"""
    cuts = [0, 100, 100, 203]
    rng = np.random.default_rng(2)
    (seg, S) = H.labelField('A', rng)
    plane = _planes(np.int16, seg, [7, None, 7], rng)[0]
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
    hist[0] = 0
    (results, errors) = H.runRankThreads(3, _oneEntryBody(seg, plane, 7, hist, np.int16, 3, cuts=cuts, bandsToo=False))
    assert not any(errors), errors
    (wic, wfc) = oracle.segstats(seg, plane, ONE_SEL, 7, -9999, max_seg_id=S)
    strad = (set(np.unique(seg[:100]).tolist()) & set(np.unique(seg[100:]).tolist())) - {0}
    assert len(strad) >= 50
    for (r, (_none, (ic, fc, nStrad, nPix))) in enumerate(results):
        assert (nStrad, nPix) == (len(strad), int(np.isin(seg, sorted(strad)).sum())), r
        assert _sameBits(ic, wic) and _sameBits(fc, wfc), r


def test_stale_histogram_raises_through_device_stats():
    """the one-band call refuses a histogram that gives an id fewer pixels than a rank holds of it, as the several-band
    call does: every rank raises, none is left in a collective"""
    from pyshepseg_amd import _lib
    rng = np.random.default_rng(5)
    (seg, S) = H.labelField('B', rng)
    plane = _planes(np.uint16, seg, NULL_FORMS['none'], rng)[0]
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
    hist[0] = 0
    cnt = H.countField(seg, S, 2)
    victim = sorted(cnt['held'][1] - cnt['strad'])[0]                  # whole on the last rank
    assert hist[victim] > 1
    hist[victim] -= 1
    (results, errors) = H.runRankThreads(2, _oneEntryBody(seg, plane, None, hist, np.uint16, 2, bandsToo=False),
                                         timeout=120)
    assert results == [None] * 2
    for (r, e) in enumerate(errors):
        assert isinstance(e, _lib.ShepsegHipError), (r, e)
        assert '1 segment ids have more pixels' in str(e), (r, e)


def _checkDriverRun(world, tmp_path, path, oracle):
    import dist_worker_stats_bands_gpu as W
    from pyshepseg_amd import tilingstats
    parts = [np.load(tmp_path / ('rank%d.npz' % r)) for r in range(world)]
    mosaic = np.zeros((1500, 1300), dtype=np.uint32)
    for q in parts:
        (lo, hi) = (int(q['outLo']), int(q['outHi']))
        mosaic[lo:hi] = np.maximum(mosaic[lo:hi], q['out'])
    S = int(parts[0]['maxSegId'])
    img = oracle.synthimg(11, 6, 1500, 1300)
    (fast, _b, nInt, nFloat) = tilingstats.makeBandStatsSelection([(b, W.selectionOf(b)) for b in W.BANDS])
    for r in range(world):
        st = np.load(tmp_path / ('bands%d.npz' % r))
        assert str(st['path']) == path and int(st['bands']) == 3
        assert np.array_equal(st['fast'], fast)
        assert st['ic'].shape == (nInt, S + 1) and st['fc'].shape == (nFloat, S + 1)
        first = 0
        for b in W.BANDS:
            sel = W.selectionOf(b)
            assert str(st['path%d' % b]) == path
            assert int(st['straddlers%d' % b]) == int(st['straddlers'])
            assert int(st['straddler_pixels%d' % b]) == int(st['straddler_pixels'])
            (wic, wfc) = oracle.segstats(mosaic, np.ascontiguousarray(img[b - 1]), sel, None, -9999, max_seg_id=S)
            own = tilingstats.makeFastStatsSelection(list(range(len(sel))), sel)[0]
            for (row, o, s) in zip(fast[first:first + len(sel)], own, sel):
                isInt = row[tilingstats.STATSEL_COLTYPE] == tilingstats.STAT_DTYPE_INT
                col = (st['ic'] if isInt else st['fc'])[row[tilingstats.STATSEL_COLARRAYINDEX]]
                idx = o[tilingstats.STATSEL_COLARRAYINDEX]
                assert _sameBits(col, (st['ic%d' % b] if isInt else st['fc%d' % b])[idx]), ('one band', r, b, s)
                assert _sameBits(col, (wic if isInt else wfc)[idx]), ('oracle', r, b, s)
            first += len(sel)
        if world > 1:
            assert int(st['straddlers']) > 0
        assert int(st['exchange_bytes']) == int(st['straddler_pixels']) * (4 + 3 * 2)


@pytest.mark.parametrize('world,transport,path', [(2, 'socket', 'host'), (1, 'rccl', 'device')])
def test_through_the_driver(world, transport, path, tmp_path, oracle):
    """the synthetic 6-band 1500 x 1300 raster through runDistributed with the HIP engine; bands 1, 3, 6 in one call
    == one call per band from the same run == the oracle on the assembled mosaic.  Two socket ranks sharing GPU 0
    take the host path with HipEngine's ...Bands methods, RCCL at world size 1 the device path."""
    dist_cases.runRanks(world, [os.path.join(ROOT, 'tests', 'dist_worker_stats_bands_gpu.py'), str(tmp_path), transport],
                        tmp_path, 900)
    _checkDriverRun(world, tmp_path, path, oracle)


def test_from_files_world_one(tmp_path, oracle):
    """doTiledShepherdSegmentationDistributed from a .npy raster with bands 2, 4, 5 selected, output kept; the
    statistics' band numbers are positions in bandNumbers.  Against calcPerSegmentStatsTiledBands on the written
    label file."""
    from pyshepseg_amd import distributed, tiling, tilingstats
    img = oracle.synthimg(11, 6, 1500, 1300)
    np.save(tmp_path / 'img.npy', img)
    bandNumbers = [2, 4, 5]
    entries = [(1, [('m1', 'mean'), ('n1', 'pixcount')]), (3, [('sd3', 'stddev'), ('med3', 'median')]),
               (2, [('min2', 'min'), ('p2', 'percentile', 75)]), (1, [('mode1', 'mode'), ('max1', 'max')])]
    cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=3)
    res = distributed.doTiledShepherdSegmentationDistributed(
        str(tmp_path / 'img.npy'), str(tmp_path / 'out.npy'), tileSize=512, overlapSize=128, minSegmentSize=50,
        numClusters=30, fixedKMeansInit=True, bandNumbers=bandNumbers, concurrencyCfg=cfg, keepOutput=True)
    try:
        info = {}
        (ic, fc, fast) = distributed.calcPerSegmentStatsDistributedBands(res.engine, res.engine.comm, res.hist, entries,
                                                                         info=info)
    finally:
        res.engine.release()
    assert info['bands'] == 3 and info['straddlers'] == 0
    sub = np.ascontiguousarray(img[[b - 1 for b in bandNumbers]])
    ref = tilingstats.calcPerSegmentStatsTiledBands(sub, entries, str(tmp_path / 'out.npy'))
    flat = [s for (_b, sel) in entries for s in sel]
    assert len(fast) == len(flat)
    for (row, s) in zip(fast, flat):
        isInt = row[tilingstats.STATSEL_COLTYPE] == tilingstats.STAT_DTYPE_INT
        col = (ic if isInt else fc)[row[tilingstats.STATSEL_COLARRAYINDEX]]
        assert np.array_equal(col, ref.columns[s[0]]), s
