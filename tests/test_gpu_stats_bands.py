"""GPU: calcPerSegmentStatsTiledBands (several bands in one pass over the labels) gives, column for column,
the bits of (1) calcPerSegmentStatsTiled called for that band and selection on its own and (2) the oracle's
orc_segstats for that band: int64 columns equal, float32 columns equal as bit patterns, no tolerance."""
import ctypes

import numpy as np
import pytest

from segtable_cases import _linear
from test_gdal_double import gdal, make_image  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ALL8 = ['min', 'max', 'mean', 'stddev', 'median', 'mode', 'pixcount']
DTYPES = ['uint8', 'int16', 'uint16', 'int32', 'uint32']


def sel_all(prefix, pcs=(25, 90)):
    """all eight statistics, the percentile with every parameter of pcs"""
    return [(prefix + s, s) for s in ALL8] + [('%sp%d' % (prefix, p), 'percentile', p) for p in pcs]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)


def check_against_single_and_oracle(oracle, img, seg, bandSelections, nulls, got, **kw):
    """got.columns against calcPerSegmentStatsTiled per entry and against the oracle per entry"""
    from pyshepseg_amd import tilingstats as ts
    names = [s[0] for (_b, sel) in bandSelections for s in sel]
    assert sorted(got.columns) == sorted(names)
    for (k, (b, sel)) in enumerate(bandSelections):
        one = ts.calcPerSegmentStatsTiled(img, b, seg, sel, imgNullVal=nulls[k], **kw)
        (fast, _ni, _nf) = ts.makeFastStatsSelection(list(range(len(sel))), sel)
        S = len(one.columns[sel[0][0]]) - 1
        (wi, wf) = oracle.segstats(seg, img[b - 1], sel, nulls[k], -9999, max_seg_id=S)
        for (i, s) in enumerate(sel):
            col = got.columns[s[0]]
            assert col.dtype == (np.float32 if s[1] in ('mean', 'stddev') else np.int64), s
            assert same_bits(col, one.columns[s[0]]), ('single-band call', k, b, s)
            want = (wf if fast[i, ts.STATSEL_COLTYPE] == ts.STAT_DTYPE_FLOAT else wi)[fast[i, ts.STATSEL_COLARRAYINDEX]]
            assert same_bits(col, want), ('oracle', k, b, s)


def ragged_labels(nr=203, nc=331):
    """test_gpu_stats' ragged raster: 5 x 7 segments that straddle the 32 x 64 patches, one far too long for a
    thread's sort, null rows"""
    seg = ((np.arange(nr)[:, None] // 5) * 100 + np.arange(nc)[None, :] // 7 + 1).astype(np.uint32)
    seg[40:90, 100:260] = 7
    seg[:3] = 0
    return seg


def block_labels(nr=203, nc=331):
    """aligned 4 x 8 blocks: every segment complete in its patch"""
    return ((np.arange(nr)[:, None] // 4) * ((nc + 7) // 8) + np.arange(nc)[None, :] // 8 + 1).astype(np.uint32)


def giant_labels():
    """test_gpu_stats' giant raster: one segment of 1.9 M pixels (k_seg_stats_big) among 300-pixel ones"""
    seg = np.ones((1500, 1500), dtype=np.uint32)
    seg[:250] = (np.arange(250 * 1500).reshape(250, 1500) // 300 + 2).astype(np.uint32)
    seg[700:720, 100:900] = 0
    return seg


def bands_of(oracle, dtype, nb, shape, seed=23):
    """nb planes of `dtype` that use its range: ties (uint8), negative values, values that need all 32 bits"""
    base = oracle.synthimg(seed, nb, shape[0], shape[1]).astype(np.int64)
    if dtype == 'uint8':
        img = (base >> 5).astype(np.uint8)
    elif dtype == 'int16':
        img = (base - 32768).astype(np.int16)
    elif dtype == 'uint16':
        img = base.astype(np.uint16)
    elif dtype == 'int32':
        img = ((base - 2720) * 2500000).astype(np.int32)
        img[:, ::3, ::2] = img[:, :1, :1]
    else:
        img = (base * 1200000).astype(np.uint32)
        img[:, 1::3, ::2] = np.uint32(0xFFFFFFFF)
    return np.ascontiguousarray(img)


@pytest.mark.parametrize('nullmode', ['none', 'one', 'perband'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_bands_every_dtype_and_null_form(dtype, nullmode, oracle):
    """3-4 bands of every library dtype: no null value, one for all bands, and one per band with a segment that is
    entirely null in ONE band only (missing / pixcount 0 there, ordinary rows in the other bands)"""
    from pyshepseg_amd import tilingstats as ts
    seg = ragged_labels()
    nb = 4 if dtype in ('uint8', 'uint16') else 3
    img = bands_of(oracle, dtype, nb, seg.shape)
    bandSelections = [(b + 1, sel_all('b%d_' % (b + 1))) for b in range(nb)]
    if nullmode == 'none':
        (nulls, arg) = ([None] * nb, None)
    elif nullmode == 'one':
        v = int(img[0, 3, 5])
        (nulls, arg) = ([v] * nb, v)
    else:
        nulls = [int(img[b, 3 + b, 5]) for b in range(nb)]
        nulls[nb - 1] = None                                    # (and one band without a null value)
        arg = list(nulls)
        # segment 7 (8000 pixels: the sorts) and a 35-pixel segment (one patch) are all null in band 2 only
        small = int(seg[100, 20])
        assert (seg == small).sum() == 35
        img[1][(seg == 7) | (seg == small)] = nulls[1]
    got = ts.calcPerSegmentStatsTiledBands(img, bandSelections, seg, imgNullVal=arg)
    check_against_single_and_oracle(oracle, img, seg, bandSelections, nulls, got)
    if nullmode == 'perband':
        for s in (7, small):
            assert got.columns['b2_pixcount'][s] == 0 and got.columns['b2_min'][s] == -9999
            assert got.columns['b2_mean'][s] == np.float32(-9999) and got.columns['b2_p90'][s] == -9999
            assert got.columns['b1_pixcount'][s] > 0 and got.columns['b%d_pixcount' % nb][s] == (seg == s).sum()
            assert got.columns['b1_min'][s] != -9999


def test_bands_different_selections_per_band(oracle):
    """one band with all eight statistics and two percentiles, one with pixcount only, one band listed twice (with
    two null values); N = 1 is the existing function"""
    from pyshepseg_amd import tilingstats as ts
    seg = ragged_labels()
    img = bands_of(oracle, 'uint16', 3, seg.shape, seed=5)
    bandSelections = [(2, sel_all('x_', (10, 75))), (3, [('n3', 'pixcount')]),
                      (1, [('m1', 'mean'), ('p1', 'percentile', 0)]), (2, [('again_sd', 'stddev'), ('again_n', 'pixcount')])]
    nulls = [int(img[1, 0, 0]), None, int(img[0, 9, 9]), int(img[1, 50, 50])]
    got = ts.calcPerSegmentStatsTiledBands(img, bandSelections, seg, imgNullVal=nulls)
    check_against_single_and_oracle(oracle, img, seg, bandSelections, nulls, got)
    for (k, (b, sel)) in enumerate(bandSelections):
        one = ts.calcPerSegmentStatsTiledBands(img, [(b, sel)], seg, imgNullVal=nulls[k])
        ref = ts.calcPerSegmentStatsTiled(img, b, seg, sel, imgNullVal=nulls[k])
        assert sorted(one.columns) == sorted(ref.columns)
        for name in ref.columns:
            assert same_bits(one.columns[name], ref.columns[name]), (k, name)


@pytest.mark.parametrize('labels', ['blocks', 'ragged', 'giant', 'linear'])
@pytest.mark.parametrize('flag', ['0', '1'])
def test_bands_patch_knob(flag, labels, oracle, monkeypatch):
    """SHEPSEG_STATS_PATCH = 0 (the sorts only) and = 1 (patches whatever the segment size): small aligned segments,
    segments that straddle patches, one giant segment (k_seg_stats_big), and runs of 1 to 10 007 pixels with
    shuffled ids"""
    from pyshepseg_amd import tilingstats as ts
    monkeypatch.setenv('SHEPSEG_STATS_PATCH', flag)
    seg = {'blocks': block_labels, 'ragged': ragged_labels, 'giant': giant_labels,
           'linear': lambda: _linear(np.repeat((1, 2, 7, 8, 9, 63, 64, 65, 511, 513, 4096, 10007), 3), 97, 1)}[labels]()
    rng = np.random.RandomState(12)
    if labels == 'giant':
        img = rng.randint(0, 900, size=(3,) + seg.shape).astype(np.uint16)      # few distinct values: long runs
        img[:, 300:1400:7] = 65535
        nulls = [None, 65535, 3]
    else:
        img = bands_of(oracle, 'uint16', 3, seg.shape, seed=19)
        for b in range(3):
            img[b][rng.rand(*seg.shape) < 0.05] = 0
        nulls = [0, None, 0]
    bandSelections = [(b + 1, sel_all('b%d_' % (b + 1), (25, 0))) for b in range(3)]
    got = ts.calcPerSegmentStatsTiledBands(img, bandSelections, seg, imgNullVal=nulls)
    check_against_single_and_oracle(oracle, img, seg, bandSelections, nulls, got)


def streamed_labels():
    """test_gpu_stats' streamed raster: 7 x 9 segments, a big one across many row blocks, an id without pixels"""
    seg = (np.arange(300)[:, None] // 7 * 60 + np.arange(400)[None, :] // 9 + 1).astype(np.uint32)
    seg[100:220, 50:300] = 77
    seg[seg == 300] = 301
    seg[seg == 1234] = 0
    seg[:3] = 0
    return seg


@pytest.mark.parametrize('flag', [None, '0'])
def test_bands_row_blocks_and_carry(flag, oracle, monkeypatch):
    """row blocks of 5 rows (60 blocks: most segments straddle one and are carried), 64 rows (5 blocks) and the
    default; RAT pages of 100 rows written once each; an id without pixels"""
    from pyshepseg_amd import tilingstats as ts
    monkeypatch.setattr(ts, 'RAT_PAGE_SIZE', 100)
    if flag is not None:
        monkeypatch.setenv('SHEPSEG_STATS_PATCH', flag)
    seg = streamed_labels()
    S = int(seg.max())
    rng = np.random.RandomState(5)
    img = bands_of(oracle, 'int16', 3, seg.shape)
    for b in range(3):
        img[b][rng.rand(*seg.shape) < 0.05] = 7 + b
    bandSelections = [(1, sel_all('a_')), (3, sel_all('c_', (10,))), (2, [('b_n', 'pixcount'), ('b_sd', 'stddev')])]
    nulls = [7, 9, 8]
    for chunk in (400 * 5, 400 * 64, None):
        got = ts.calcPerSegmentStatsTiledBands(img, bandSelections, seg, imgNullVal=nulls, chunkPixels=chunk)
        check_against_single_and_oracle(oracle, img, seg, bandSelections, nulls, got, chunkPixels=chunk)
        starts = [p[0] for p in got.pagesWritten]
        assert sorted(starts) == list(range(0, S + 1, 100)) and len(set(starts)) == len(starts)
        assert dict(got.pagesWritten)[max(starts)] == S + 1 - max(starts)
        assert got.columns['a_pixcount'][300] == 0 and got.columns['c_min'][300] == -9999
        assert got.columns['b_sd'][300] == np.float32(-9999)
    assert set(got.timings.makeSummaryDict()) >= {'reading', 'accumulation', 'statscompletion', 'writing'}


def test_bands_counts_the_labels_once(oracle, monkeypatch):
    """without segSize the label histogram is counted once per call, whatever the number of bands"""
    from pyshepseg_amd import tilingstats as ts
    seg = block_labels(64, 96)
    img = bands_of(oracle, 'uint8', 4, seg.shape)
    calls = []
    real = ts._countSegments
    monkeypatch.setattr(ts, '_countSegments', lambda *a: (calls.append(1), real(*a))[1])
    bandSelections = [(b + 1, [('m%d' % b, 'mean'), ('n%d' % b, 'pixcount')]) for b in range(4)]
    got = ts.calcPerSegmentStatsTiledBands(img, bandSelections, seg)
    assert len(calls) == 1
    ts.calcPerSegmentStatsTiled(img, 2, seg, bandSelections[1][1])          # (the one-band call: the same code)
    assert len(calls) == 2
    monkeypatch.setattr(ts, '_countSegments', real)
    check_against_single_and_oracle(oracle, img, seg, bandSelections, [None] * 4, got)


def test_bands_npy_paths(oracle, tmp_path):
    """.npy paths: the image memory-mapped, band planes read block by block"""
    from pyshepseg_amd import tilingstats as ts
    seg = ragged_labels()
    img = bands_of(oracle, 'uint16', 4, seg.shape, seed=8)
    np.save(str(tmp_path / 'img.npy'), img)
    np.save(str(tmp_path / 'seg.npy'), seg)
    bandSelections = [(4, sel_all('d_')), (1, sel_all('a_')), (2, [('b_n', 'pixcount')])]
    nulls = [int(img[3, 0, 0]), None, int(img[1, 0, 0])]
    for chunk in (331 * 40, None):
        got = ts.calcPerSegmentStatsTiledBands(str(tmp_path / 'img.npy'), bandSelections, str(tmp_path / 'seg.npy'),
                                               imgNullVal=nulls, chunkPixels=chunk)
        check_against_single_and_oracle(oracle, img, seg, bandSelections, nulls, got)


def test_bands_on_device_resident_rasters(oracle):
    """tiling.DeviceRaster + a segmentation kept in HBM: no raster is copied; the raster's null value is the default
    of every band; a short segSize is refused"""
    from pyshepseg_amd import _lib, tiling, tilingstats as ts
    ras = tiling.DeviceRaster.synth(3, 4, 700, 900)
    bandSelections = [(2, sel_all('b2_')), (4, [('b4_m', 'mean'), ('b4_n', 'pixcount')]), (1, sel_all('b1_', (50,)))]
    try:
        cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=3)
        kw = dict(tileSize=256, overlapSize=64, minSegmentSize=30, numClusters=12, fixedKMeansInit=True,
                  concurrencyCfg=cfg)
        rd = tiling.doTiledShepherdSegmentation(ras, tiling._KEEP_ON_DEVICE, **kw)
        img = ras.toArray()
        nulls = [int(img[1, 0, 0]), None, int(img[0, 0, 0])]
        got = ts.calcPerSegmentStatsTiledBands(ras, bandSelections, rd, imgNullVal=nulls)
        gotChunked = ts.calcPerSegmentStatsTiledBands(ras, bandSelections, rd, imgNullVal=nulls, chunkPixels=900 * 100)
        single = [ts.calcPerSegmentStatsTiled(ras, b, rd, sel, imgNullVal=nulls[k])
                  for (k, (b, sel)) in enumerate(bandSelections)]
        with pytest.raises(ts.PyShepSegStatsError, match='segSize has'):
            ts.calcPerSegmentStatsTiledBands(ras, bandSelections, rd, segSize=np.asarray(rd.hist)[:-1])
        with pytest.raises(ts.PyShepSegStatsError, match='band 5 not in image'):
            ts.calcPerSegmentStatsTiledBands(ras, [(1, [('a', 'min')]), (5, [('b', 'min')])], rd)
        with pytest.raises(ts.PyShepSegStatsError, match='different sizes'):
            small = tiling.DeviceRaster.synth(3, 1, 64, 64)
            try:
                ts.calcPerSegmentStatsTiledBands(small, [(1, [('a', 'min')])], rd)
            finally:
                small.free()
        segimg = np.empty((700, 900), dtype=np.uint32)
        c = _lib.ctx()
        c.check(c._L.shp_dev_download(c.handle, segimg.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(rd.outDev[0]),
                                      segimg.nbytes))
        tiling.freeDeviceOutput(rd)
    finally:
        ras.free()
    for (k, (_b, sel)) in enumerate(bandSelections):
        for s in sel:
            assert same_bits(got.columns[s[0]], single[k].columns[s[0]]), s
            assert same_bits(gotChunked.columns[s[0]], single[k].columns[s[0]]), s
    check_against_single_and_oracle(oracle, img, segimg, bandSelections, nulls, got, segSize=np.asarray(rd.hist))


def test_bands_through_gdal(gdal, oracle, monkeypatch):  # noqa: F811
    """file names: every band's own nodata value, the Histogram column as segSize, all columns of all bands into the
    segment file's attribute table, a page (100 rows here) leaving with all its columns together"""
    from pyshepseg_amd import tilingstats as ts
    monkeypatch.setattr(ts, 'RAT_PAGE_SIZE', 100)
    seg = streamed_labels()
    S = int(seg.max())
    img = bands_of(oracle, 'uint16', 3, seg.shape, seed=31)
    nodata = [int(img[0, 0, 0]), int(img[1, 200, 200]), int(img[2, 5, 5])]
    make_image(gdal, 'img.kea', img, nodata)
    segds = make_image(gdal, 'seg.kea', seg[None], 0)
    rat = segds.GetRasterBand(1).GetDefaultRAT()
    bandSelections = [(1, sel_all('b1_')), (3, [('b3_mean', 'mean'), ('b3_n', 'pixcount')]), (2, sel_all('b2_', (5,)))]
    with pytest.raises(ts.PyShepSegStatsError, match='Histogram column must exist'):
        ts.calcPerSegmentStatsTiledBands('img.kea', bandSelections, 'seg.kea')
    rat.SetRowCount(S + 1)
    rat.CreateColumn('Histogram', gdal.GFT_Real, gdal.GFU_PixelCount)
    rat.WriteArray(np.bincount(seg.reshape(-1), minlength=S + 1).astype(np.float64), 0)
    del gdal.CALLS[:]
    for chunk in (400 * 64, None):
        res = ts.calcPerSegmentStatsTiledBands('img.kea', bandSelections, 'seg.kea', chunkPixels=chunk)
        assert res.columns is None                                                  # they went to the file
        names = [rat.GetNameOfCol(i) for i in range(rat.GetColumnCount())]
        want = ts.calcPerSegmentStatsTiledBands(img, bandSelections, seg, imgNullVal=[nodata[0], nodata[2], nodata[1]])
        check_against_single_and_oracle(oracle, img, seg, bandSelections, [nodata[0], nodata[2], nodata[1]], want)
        flat = [s for (_b, sel) in bandSelections for s in sel]
        assert names == ['Histogram'] + [s[0] for s in flat]
        for s in flat:
            i = names.index(s[0])
            isFloat = s[1] in ('mean', 'stddev')
            assert rat.GetTypeOfCol(i) == (gdal.GFT_Real if isFloat else gdal.GFT_Integer)
            assert np.array_equal(rat.ReadAsArray(i)[1:], want.columns[s[0]][1:].astype(np.float64 if isFloat else np.int64)), s
        # a page is written with all its columns one after the other, in column order, once
        writes = [cl for cl in gdal.CALLS if cl[0] == 'RAT.WriteArray']
        assert len(writes) == len(flat) * len(range(0, S + 1, 100))
        for p in range(0, len(writes), len(flat)):
            page = writes[p:p + len(flat)]
            assert [w[1] for w in page] == list(range(1, len(flat) + 1))
            assert len(set(w[2] for w in page)) == 1 and page[0][2] % 100 == 0
        assert sorted(set(w[2] for w in writes)) == list(range(0, S + 1, 100))
        del gdal.CALLS[:]


def test_bands_errors(oracle):
    from pyshepseg_amd import tilingstats as ts
    seg = block_labels(32, 64)
    img = bands_of(oracle, 'uint16', 2, seg.shape)
    two = [(1, [('a', 'mean')]), (2, [('b', 'min')])]
    with pytest.raises(ts.PyShepSegStatsError, match='Float image types'):
        ts.calcPerSegmentStatsTiledBands(img.astype(np.float32), two, seg)
    with pytest.raises(ts.PyShepSegStatsError, match='different sizes'):
        ts.calcPerSegmentStatsTiledBands(img[:, :, :60], two, seg)
    with pytest.raises(ts.PyShepSegStatsError, match='band 3 not in image'):
        ts.calcPerSegmentStatsTiledBands(img, [(1, [('a', 'mean')]), (3, [('b', 'min')])], seg)
    with pytest.raises(ts.PyShepSegStatsError, match='imgNullVal has'):
        ts.calcPerSegmentStatsTiledBands(img, two, seg, imgNullVal=[1, 2, 3])
    with pytest.raises(ts.PyShepSegStatsError, match='more than once'):
        ts.calcPerSegmentStatsTiledBands(img, [(1, [('a', 'mean')]), (2, [('a', 'min')])], seg)
    with pytest.raises(ts.PyShepSegStatsError, match='selects no statistic'):
        ts.calcPerSegmentStatsTiledBands(img, [(1, [('a', 'mean')]), (2, [])], seg)
    with pytest.raises(ts.PyShepSegStatsError):
        ts.calcPerSegmentStatsTiledBands(img, [], seg)


def test_c5_stats_bands_fullsize(oracle):
    """the C5 geometry (1.6 Gpx of 4 x 8-pixel blocks, 50 M segments) with three uint16 bands in one call against
    three one-band calls: every column bit for bit; every pixel counted once in every band"""
    from pyshepseg_amd import tiling, tilingstats, _lib
    N, BH, BW, NB = 40000, 4, 8, 3
    c = _lib.ctx()
    ras = tiling.DeviceRaster.synth(11, NB, N, N)
    d_seg = ctypes.c_void_p()
    c.check(c._L.shp_dev_alloc(c.handle, N * N * 4, ctypes.byref(d_seg)))
    try:
        S = ctypes.c_uint32(0)
        c.check(c._L.shp_dev_block_labels(c.handle, N, N, BH, BW, d_seg, ctypes.byref(S)))
        S = S.value
        assert S == 50000000
        sel = [('mean', 'mean'), ('sd', 'stddev'), ('med', 'median'), ('n', 'pixcount')]
        bandSelections = [(b + 1, [('b%d_%s' % (b + 1, s[0]),) + s[1:] for s in sel]) for b in range(NB)]
        (fast, bandOfStat, ni, nf) = tilingstats.makeBandStatsSelection(bandSelections)
        ic = np.zeros((ni, S + 1), dtype=np.int64)
        fc = np.zeros((nf, S + 1), dtype=np.float32)
        planes = (ctypes.c_void_p * NB)(*[ras.ptr + b * N * N * 2 for b in range(NB)])
        hasNull = np.zeros(NB, dtype=np.int32)
        nullVal = np.zeros(NB, dtype=np.int64)
        perBand = np.full(NB, len(sel), dtype=np.int32)
        c.check(c._L.shp_segstats2d_bands_dev(c.handle, d_seg, planes, 2, NB, N, N, S, _lib.ptr(hasNull), _lib.ptr(nullVal),
                                              _lib.ptr(fast), _lib.ptr(perBand), -9999, _lib.ptr(ic), _lib.ptr(fc)))
        (f1, n1i, n1f) = tilingstats.makeFastStatsSelection(list(range(len(sel))), sel)
        ic1 = np.zeros((n1i, S + 1), dtype=np.int64)
        fc1 = np.zeros((n1f, S + 1), dtype=np.float32)
        for b in range(NB):
            c.check(c._L.shp_segstats2d_dev(c.handle, d_seg, ctypes.c_void_p(planes[b]), 2, N, N, S, 0, 0, _lib.ptr(f1),
                                            len(sel), -9999, _lib.ptr(ic1), _lib.ptr(fc1)))
            for (own, comb) in zip(f1, fast[bandOfStat == b]):
                if own[2] == 0:
                    assert np.array_equal(ic[comb[3]], ic1[own[3]]), (b, own)
                else:
                    assert np.array_equal(fc[comb[3]].view(np.uint32), fc1[own[3]].view(np.uint32)), (b, own)
            npx = ic1[f1[3, 3]]
            assert int(npx.sum()) == N * N and npx[0] == 0 and (npx[1:] == BH * BW).all()
        assert not np.array_equal(fc[0], fc[2])                 # (the bands differ)
    finally:
        c.check(c._L.shp_dev_free(c.handle, d_seg))
        ras.free()
