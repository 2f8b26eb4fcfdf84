"""GPU: pyshepseg_amd.utils.writeColorTableFromRatColumns and renderColourTable.

The expected colour bytes are the reference's expression (pyshepseg/utils.py:216-221) evaluated by numpy in the
test, on the column as a RAT hands it over (float64, or int64 for Integer columns):

    lo, hi = numpy.percentile(col, 5), numpy.percentile(col, 95)
    clr = (255 * ((col - lo) / (hi - lo)).clip(0, 1)).astype(numpy.uint8)

No tolerance: numpy.array_equal on the byte columns, == on lo and hi.  The expected rendering is
numpy.stack([R[seg], G[seg], B[seg], A[seg]], -1)."""
import ctypes

import numpy as np
import pytest

from test_gdal_double import gdal, make_image  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 20, 1000, 100003, (1 << 20) + 7]
KINDS = ['uniform', 'means16', 'missing30', 'mixedsign', 'int64']


def reference_bytes(col):
    """utils.py:216-221 on a float64 / int64 column"""
    col = np.asarray(col)
    assert col.dtype in (np.float64, np.int64)
    lo = np.percentile(col, 5)
    hi = np.percentile(col, 95)
    with np.errstate(divide='ignore', invalid='ignore'):
        clr = (255 * ((col - lo) / (hi - lo)).clip(0, 1))
        return (lo, hi, clr.astype(np.uint8))


def column(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == 'uniform':
        return rng.random(n) * 4000.0
    if kind == 'means16':           # integer sum over integer count: many exact ties
        cnt = rng.integers(1, 12, n)
        return (rng.integers(0, 300, n) * cnt // 3).astype(np.float64) / cnt.astype(np.float64)
    if kind == 'missing30':         # the 5th percentile falls inside the run of missing values
        col = rng.random(n) * 9000.0 + 100.0
        col[rng.random(n) < 0.3] = -9999.0
        if n >= 20:
            col[:n // 3] = -9999.0
        return col
    if kind == 'mixedsign':
        col = rng.standard_normal(n) * 1e3
        col[::7] = -col[::7] * 1e-300           # denormals and tiny values of both signs
        col[::11] = 0.0
        col[::13] = -0.0
        return col
    return rng.integers(-40000, 70000, n).astype(np.int64)


def check_table(got, cols, names):
    for (name, colour, lohi) in zip(names, ('Red', 'Green', 'Blue'), got.stretch):
        src = np.asarray(cols[name])
        if src.dtype.kind == 'f':
            src = src.astype(np.float64)            # (what a RAT returns for a Real column; exact)
        (lo, hi, want) = reference_bytes(src)
        print(name, len(src), 'lo', lohi[0], lo, 'hi', lohi[1], hi, 'bytes differ', int((got.columns[colour] != want).sum()))
        assert lohi[0] == lo and lohi[1] == hi, (name, lohi, lo, hi)
        assert got.columns[colour].dtype == np.uint8
        assert np.array_equal(got.columns[colour], want), name
    assert got.columns['Alpha'].dtype == np.uint8 and (got.columns['Alpha'] == 255).all()
    assert len(got.columns['Alpha']) == len(got.columns['Red'])
    assert sorted(got.columns) == ['Alpha', 'Blue', 'Green', 'Red']


@pytest.mark.parametrize('n', LENGTHS)
def test_columns_equal_numpy(n):
    """every length with every kind of column, three at a time"""
    from pyshepseg_amd import utils
    cols = {k: column(k, n, 100 + i) for (i, k) in enumerate(KINDS)}
    cols['uniform2'] = column('uniform', n, 7) - 2000.0
    for names in (('uniform', 'means16', 'missing30'), ('mixedsign', 'int64', 'uniform2')):
        got = utils.writeColorTableFromRatColumns(cols, *names)
        check_table(got, cols, names)
        assert got.deviceMs > 0


def test_float32_and_small_integer_columns():
    """the statistics' own column types: float32 means are widened exactly, integer columns of any width go as int64"""
    from pyshepseg_amd import utils
    rng = np.random.default_rng(3)
    n = 5000
    cols = {'f32': (rng.random(n) * 3000).astype(np.float32), 'i32': rng.integers(-9999, 60000, n).astype(np.int32),
            'u16': rng.integers(0, 65535, n).astype(np.uint16)}
    got = utils.writeColorTableFromRatColumns(cols, 'f32', 'i32', 'u16')
    check_table(got, {'f32': cols['f32'], 'i32': cols['i32'].astype(np.int64), 'u16': cols['u16'].astype(np.int64)},
                ('f32', 'i32', 'u16'))


def test_degenerate_stretch():
    """hi == lo: the reference divides by zero, and numpy on x86-64 ends with 255 where col > lo and 0 elsewhere
    (inf clips to 1, the NaN of col == lo casts to 0).  A constant column, and a column whose 5th and 95th
    percentiles coincide although it is not constant."""
    from pyshepseg_amd import utils
    n = 1000
    const = np.full(n, 1234.5)
    coincide = np.full(n, 40.0)
    coincide[:20] = -7.0
    coincide[-20:] = 900.0              # 2 % below, 2 % above: both percentiles are 40
    ints = np.full(n, 3, dtype=np.int64)
    ints[5] = 11
    ints[6] = -2
    cols = {'const': const, 'coincide': coincide, 'ints': ints}
    got = utils.writeColorTableFromRatColumns(cols, 'const', 'coincide', 'ints')
    assert got.stretch == [(1234.5, 1234.5), (40.0, 40.0), (3.0, 3.0)]
    assert (got.columns['Red'] == 0).all()
    assert np.array_equal(got.columns['Green'], np.where(coincide > 40.0, 255, 0).astype(np.uint8))
    assert got.columns['Green'].sum() == 20 * 255
    assert np.array_equal(got.columns['Blue'], np.where(ints > 3, 255, 0).astype(np.uint8))
    check_table(got, cols, ('const', 'coincide', 'ints'))           # (numpy here agrees with the documented result)


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize('n', [1, 70001])
def test_non_finite_is_refused(bad, n):
    from pyshepseg_amd import _lib, utils
    good = np.linspace(0.0, 50.0, n)
    col = good.copy()
    col[n // 2] = bad
    with pytest.raises(_lib.ShepsegHipError, match='NaN or an infinity'):
        utils.writeColorTableFromRatColumns({'a': good, 'b': col, 'c': good}, 'a', 'b', 'c')
    col32 = col.astype(np.float32)
    with pytest.raises(_lib.ShepsegHipError, match='NaN or an infinity'):
        utils.writeColorTableFromRatColumns({'a': good, 'b': good, 'c': col32}, 'a', 'b', 'c')
    got = utils.writeColorTableFromRatColumns({'a': good, 'b': good, 'c': good}, 'a', 'b', 'c')    # (the context is fine)
    check_table(got, {'a': good}, ('a', 'a', 'a'))


def test_wide_integers_are_refused():
    from pyshepseg_amd import _lib, utils
    ok = np.arange(100, dtype=np.int64)
    edge = ok.copy()
    edge[3] = (1 << 53) - 1
    edge[4] = -(1 << 53) + 1
    got = utils.writeColorTableFromRatColumns({'a': ok, 'b': edge}, 'a', 'b', 'a')
    check_table(got, {'a': ok, 'b': edge}, ('a', 'b', 'a'))
    for v in (1 << 53, -(1 << 53), np.iinfo(np.int64).max):
        wide = ok.copy()
        wide[50] = v
        with pytest.raises(_lib.ShepsegHipError, match='2\\^53'):
            utils.writeColorTableFromRatColumns({'a': ok, 'b': wide}, 'a', 'b', 'a')
    for v in (1 << 63, (1 << 64) - 1):                              # (neither wraps into range as int64)
        with pytest.raises(utils.PyShepSegUtilsError, match='2\\^53'):
            utils.writeColorTableFromRatColumns({'a': ok, 'b': np.full(5, v, dtype=np.uint64)}, 'b', 'b', 'b')
    with pytest.raises(_lib.ShepsegHipError, match='2\\^53'):
        utils.writeColorTableFromRatColumns({'a': ok, 'b': np.full(5, 1 << 60, dtype=np.uint64)}, 'b', 'b', 'b')


# ---- end to end -----------------------------------------------------------------------------------------
SCENE = (1500, 1700)


def segment_scene(oracle):
    """a synthetic 3-band scene through the tiled segmentation: a few thousand segments"""
    from pyshepseg_amd import tiling
    img = oracle.synthimg(3, 3, SCENE[0], SCENE[1])
    cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=3)
    r = tiling.doTiledShepherdSegmentation(img, None, tileSize=512, overlapSize=64, minSegmentSize=10, numClusters=12,
                                           fixedKMeansInit=True, concurrencyCfg=cfg)
    print('segments:', r.maxSegId)
    return (img, r)


MEANS = [(b, [('Band_%d_mean' % b, 'mean')]) for b in (1, 2, 3)]
MEAN_NAMES = ('Band_1_mean', 'Band_2_mean', 'Band_3_mean')


def test_pipeline_segment_stats_colour_render(oracle, tmp_path):
    """segment -> calcPerSegmentStatsTiledBands means -> colour table -> rendering, on arrays"""
    from pyshepseg_amd import tilingstats as ts, utils
    (img, r) = segment_scene(oracle)
    assert r.maxSegId >= 1000
    res = ts.calcPerSegmentStatsTiledBands(img, MEANS, r.segimg)
    got = utils.writeColorTableFromRatColumns(res, *MEAN_NAMES)
    assert len(got.columns['Red']) == r.maxSegId + 1
    check_table(got, res.columns, MEAN_NAMES)
    again = utils.writeColorTableFromRatColumns(res.columns, *MEAN_NAMES)
    for k in got.columns:
        assert np.array_equal(got.columns[k], again.columns[k])
    rgba = utils.renderColourTable(r.segimg, got)
    want = np.stack([got.columns[k][r.segimg] for k in ('Red', 'Green', 'Blue', 'Alpha')], -1)
    assert rgba.dtype == np.uint8 and rgba.shape == SCENE + (4,) and np.array_equal(rgba, want)
    assert len(np.unique(rgba.reshape(-1, 4), axis=0)) > 100          # (a picture, not a constant)


def test_pipeline_through_gdal(gdal, oracle):  # noqa: F811
    """the same through file names: the RAT ends with Red / Green / Blue / Alpha holding those bytes, created
    once, Integer, with GDAL's usages, in the reference's order; a second call reuses them"""
    from pyshepseg_amd import tilingstats as ts, utils
    (img, r) = segment_scene(oracle)
    S = int(r.maxSegId)
    make_image(gdal, 'img.kea', img, None)
    segds = make_image(gdal, 'seg.kea', r.segimg[None], 0)
    rat = segds.GetRasterBand(1).GetDefaultRAT()
    rat.SetRowCount(S + 1)
    rat.CreateColumn('Histogram', gdal.GFT_Real, gdal.GFU_PixelCount)
    rat.WriteArray(np.asarray(r.hist).astype(np.float64), 0)
    ts.calcPerSegmentStatsTiledBands('img.kea', MEANS, 'seg.kea')
    inMemory = utils.writeColorTableFromRatColumns(ts.calcPerSegmentStatsTiledBands(img, MEANS, r.segimg), *MEAN_NAMES)
    names = [rat.GetNameOfCol(i) for i in range(rat.GetColumnCount())]
    assert names == ['Histogram'] + list(MEAN_NAMES)
    held = {n: rat.ReadAsArray(names.index(n)) for n in MEAN_NAMES}
    del gdal.CALLS[:]
    got = utils.writeColorTableFromRatColumns('seg.kea', *MEAN_NAMES)
    check_table(got, held, MEAN_NAMES)
    created = [c for c in gdal.CALLS if c[0] == 'RAT.CreateColumn']
    assert created == [('RAT.CreateColumn', 'Red', 0, 6), ('RAT.CreateColumn', 'Green', 0, 7),
                       ('RAT.CreateColumn', 'Blue', 0, 8), ('RAT.CreateColumn', 'Alpha', 0, 9)]
    # each colour column is created right before it is written, whole, as in the reference
    trace = [c[:2] for c in gdal.CALLS if c[0] in ('RAT.CreateColumn', 'RAT.WriteArray')]
    assert trace == [('RAT.CreateColumn', 'Red'), ('RAT.WriteArray', 4), ('RAT.CreateColumn', 'Green'),
                     ('RAT.WriteArray', 5), ('RAT.CreateColumn', 'Blue'), ('RAT.WriteArray', 6),
                     ('RAT.CreateColumn', 'Alpha'), ('RAT.WriteArray', 7)]
    assert all(c[2:] == (0, S + 1) for c in gdal.CALLS if c[0] == 'RAT.WriteArray')
    assert any(c[0] == 'Dataset.FlushCache' for c in gdal.CALLS)
    names = [rat.GetNameOfCol(i) for i in range(rat.GetColumnCount())]
    assert names == ['Histogram'] + list(MEAN_NAMES) + ['Red', 'Green', 'Blue', 'Alpha']
    for (k, usage) in zip(('Red', 'Green', 'Blue', 'Alpha'), (6, 7, 8, 9)):
        i = names.index(k)
        assert rat.GetTypeOfCol(i) == gdal.GFT_Integer and rat.GetUsageOfCol(i) == usage
        assert np.array_equal(rat.ReadAsArray(i), got.columns[k].astype(np.int64)), k
        assert np.array_equal(got.columns[k][1:], inMemory.columns[k][1:]), k
    del gdal.CALLS[:]
    again = utils.writeColorTableFromRatColumns(gdal.Open('seg.kea', gdal.GA_Update), MEAN_NAMES[2], MEAN_NAMES[1],
                                                MEAN_NAMES[0])
    assert not [c for c in gdal.CALLS if c[0] == 'RAT.CreateColumn'] and rat.GetColumnCount() == 8
    assert [c[1] for c in gdal.CALLS if c[0] == 'RAT.WriteArray'] == [4, 5, 6, 7]
    assert np.array_equal(again.columns['Red'], got.columns['Blue'])
    assert np.array_equal(rat.ReadAsArray(names.index('Red')), got.columns['Blue'].astype(np.int64))
    # the RAT's own colour columns (int64) render as the result object does
    fromRat = {k: rat.ReadAsArray(names.index(k)) for k in ('Red', 'Green', 'Blue', 'Alpha')}
    assert np.array_equal(utils.renderColourTable(r.segimg, fromRat), utils.renderColourTable(r.segimg, again))


# ---- rendering ------------------------------------------------------------------------------------------
def labels_and_table(nr, nc, seed=2):
    rng = np.random.default_rng(seed)
    S = 5000
    seg = ((np.arange(nr)[:, None] // 3) * 41 + np.arange(nc)[None, :] // 5).astype(np.uint32) % np.uint32(S + 1)
    seg[rng.random((nr, nc)) < 0.1] = rng.integers(0, S + 1, dtype=np.uint32)
    seg[0, 0] = S
    seg[-1, -1] = 0
    colours = {k: rng.integers(0, 256, S + 1, dtype=np.uint8) for k in ('Red', 'Green', 'Blue', 'Alpha')}
    return (seg, colours)


def expected_rgba(seg, colours):
    return np.stack([np.asarray(colours[k])[seg] for k in ('Red', 'Green', 'Blue', 'Alpha')], -1).astype(np.uint8)


@pytest.mark.parametrize('shape', [(64, 128), (203, 331), (97, 1), (1, 97), (5, 2), (1, 1), (37, 1023)])
def test_render_host_array_every_width(shape):
    """widths that are and are not multiples of the kernel's four labels per lane; five and more row blocks give
    the bytes of one block"""
    from pyshepseg_amd import utils
    (seg, colours) = labels_and_table(*shape)
    want = expected_rgba(seg, colours)
    one = utils.renderColourTable(seg, colours)
    assert one.dtype == np.uint8 and one.shape == shape + (4,)
    assert np.array_equal(one, want)
    if shape[0] >= 5:
        rows = max(1, shape[0] // 6)
        assert -(-shape[0] // rows) >= 5
        assert np.array_equal(utils.renderColourTable(seg, colours, chunkPixels=rows * shape[1]), want)
        assert np.array_equal(utils.renderColourTable(seg, colours, chunkPixels=1), want)        # a row per block


def test_render_random_table_and_result_object():
    from pyshepseg_amd import utils
    (seg, _c) = labels_and_table(120, 77)
    table = utils.writeRandomColourTable(None, 5001, seed=8)
    rgba = utils.renderColourTable(seg, table)
    assert np.array_equal(rgba, expected_rgba(seg, table.columns))
    assert (rgba[seg == 0][:, 3] == 0).all() and (rgba[seg != 0][:, 3] == 255).all()


def test_render_npy_paths(tmp_path):
    """.npy in (memory-mapped, read block by block), .npy out through the row writer"""
    from pyshepseg_amd import utils
    (seg, colours) = labels_and_table(203, 331)
    want = expected_rgba(seg, colours)
    np.save(str(tmp_path / 'seg.npy'), seg)
    for (k, chunk) in enumerate((None, 331 * 40, 331 * 7 + 5)):
        out = str(tmp_path / ('rgba%d.npy' % k))
        assert utils.renderColourTable(str(tmp_path / 'seg.npy'), colours, outfile=out, chunkPixels=chunk) is None
        back = np.load(out)
        assert back.dtype == np.uint8 and back.shape == (203, 331, 4) and np.array_equal(back, want)
    out = str(tmp_path / 'fromarray.npy')
    utils.renderColourTable(seg, colours, outfile=out, chunkPixels=331 * 50)
    assert np.array_equal(np.load(out), want)


def test_render_device_resident_labels(oracle):
    """labels kept in HBM by the tiled segmentation: read in place, also from row blocks that start off a 16-byte
    boundary (the raster is 902 labels wide)"""
    from pyshepseg_amd import _lib, tiling, tilingstats as ts, utils
    ras = tiling.DeviceRaster.synth(3, 3, 300, 902)
    try:
        cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=3)
        rd = tiling.doTiledShepherdSegmentation(ras, tiling._KEEP_ON_DEVICE, tileSize=256, overlapSize=64,
                                                minSegmentSize=30, numClusters=12, fixedKMeansInit=True,
                                                concurrencyCfg=cfg)
        try:
            res = ts.calcPerSegmentStatsTiledBands(ras, MEANS, rd)
            table = utils.writeColorTableFromRatColumns(res, *MEAN_NAMES)
            check_table(table, res.columns, MEAN_NAMES)
            whole = utils.renderColourTable(rd, table)
            blocks = utils.renderColourTable(rd, table, chunkPixels=902 * 7)
            oddBlocks = utils.renderColourTable(rd, table, chunkPixels=902 * 3)
            short = {k: v[:-1] for (k, v) in table.columns.items()}
            with pytest.raises(_lib.ShepsegHipError, match='segment id %d is not in the colour table' % rd.maxSegId):
                utils.renderColourTable(rd, short)
            segimg = np.empty((300, 902), dtype=np.uint32)
            c = _lib.ctx()
            c.check(c._L.shp_dev_download(c.handle, segimg.ctypes.data_as(ctypes.c_void_p),
                                          ctypes.c_void_p(rd.outDev[0]), segimg.nbytes))
        finally:
            tiling.freeDeviceOutput(rd)
    finally:
        ras.free()
    want = expected_rgba(segimg, table.columns)
    assert np.array_equal(whole, want) and np.array_equal(blocks, want) and np.array_equal(oddBlocks, want)


def test_render_label_outside_the_table():
    """a label equal to the table's length (and beyond) raises and the message names it; nothing is read out of range"""
    from pyshepseg_amd import _lib, utils
    (seg, colours) = labels_and_table(64, 130)
    n = len(colours['Red'])
    for (where, label) in (((63, 129), n), ((0, 0), n), ((31, 2), 0xFFFFFFFF), ((10, 77), n + 12345)):
        bad = seg.copy()
        bad[where] = label
        with pytest.raises(_lib.ShepsegHipError, match='segment id %d is not in the colour table \\(%d rows\\)' % (label, n)):
            utils.renderColourTable(bad, colours)
        with pytest.raises(_lib.ShepsegHipError, match='segment id %d is not' % label):
            utils.renderColourTable(bad, colours, chunkPixels=130 * 9)
    bad = seg.copy()
    bad[5, 5] = n + 7
    bad[50, 5] = n + 3
    with pytest.raises(_lib.ShepsegHipError, match='segment id %d is not' % (n + 3)):          # the smallest one
        utils.renderColourTable(bad, colours)
    assert np.array_equal(utils.renderColourTable(seg, colours), expected_rgba(seg, colours))  # (the context is fine)
