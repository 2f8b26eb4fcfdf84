"""CPU: the host side of pyshepseg_amd.utils -- argument checks that come before any GPU work, the GDAL usage
constants, and writeRandomColourTable (which needs no kernel), in memory and through the stand-in GDAL."""
import numpy as np
import pytest

from test_gdal_double import gdal, make_image  # noqa: F401  (fixture)


def four(n, **over):
    cols = {k: np.full(n, 9, dtype=np.uint8) for k in ('Red', 'Green', 'Blue', 'Alpha')}
    cols.update(over)
    return cols


def test_gfu_constants_are_gdals():
    from pyshepseg_amd import utils
    assert (utils.GFU_Red, utils.GFU_Green, utils.GFU_Blue, utils.GFU_Alpha) == (6, 7, 8, 9)
    assert utils.GFT_Integer == 0


def test_missing_column_is_an_error_before_any_work(monkeypatch):
    """the name check comes before the GPU context is asked for (which would fail first where there is no GPU)"""
    from pyshepseg_amd import _lib, utils, tilingstats as ts
    asked = []
    monkeypatch.setattr(_lib, 'ctx', lambda: asked.append(1))
    cols = {'a': np.arange(5.0), 'b': np.arange(5.0), 'c': np.arange(5.0)}
    with pytest.raises(utils.PyShepSegUtilsError, match="'nope' is not in the table"):
        utils.writeColorTableFromRatColumns(cols, 'a', 'nope', 'c')
    res = ts.TiledStatsResult()
    res.columns = cols
    with pytest.raises(utils.PyShepSegUtilsError, match="'d' is not in the table"):
        utils.writeColorTableFromRatColumns(res, 'a', 'b', 'd')
    res.columns = None
    with pytest.raises(utils.PyShepSegUtilsError, match='went to the segment file'):
        utils.writeColorTableFromRatColumns(res, 'a', 'b', 'c')
    cols['c'] = np.arange(6.0)
    with pytest.raises(utils.PyShepSegUtilsError, match='differ in length'):
        utils.writeColorTableFromRatColumns(cols, 'a', 'b', 'c')
    assert asked == []


def test_missing_column_through_gdal(gdal, monkeypatch):  # noqa: F811
    from pyshepseg_amd import _lib, utils
    asked = []
    monkeypatch.setattr(_lib, 'ctx', lambda: asked.append(1))
    segds = make_image(gdal, 'seg.kea', np.zeros((1, 4, 4), dtype=np.uint32), 0)
    rat = segds.GetRasterBand(1).GetDefaultRAT()
    rat.SetRowCount(3)
    rat.CreateColumn('m1', gdal.GFT_Real, gdal.GFU_Generic)
    rat.CreateColumn('m2', gdal.GFT_Real, gdal.GFU_Generic)
    del gdal.CALLS[:]
    for segfile in ('seg.kea', segds):
        with pytest.raises(utils.PyShepSegUtilsError, match="'m3' is not in the table"):
            utils.writeColorTableFromRatColumns(segfile, 'm1', 'm2', 'm3')
    assert asked == [] and not [c for c in gdal.CALLS if c[0] in ('RAT.CreateColumn', 'RAT.WriteArray')]


def test_render_refuses_bad_colours(monkeypatch):
    from pyshepseg_amd import _lib, utils
    asked = []
    monkeypatch.setattr(_lib, 'ctx', lambda: asked.append(1))
    seg = np.zeros((4, 4), dtype=np.uint32)
    with pytest.raises(utils.PyShepSegUtilsError, match="'Alpha' has 4 rows, 'Red' has 5"):
        utils.renderColourTable(seg, four(5, Alpha=np.full(4, 255, dtype=np.uint8)))
    for name in ('Red', 'Green', 'Blue', 'Alpha'):
        cols = four(5)
        del cols[name]
        with pytest.raises(utils.PyShepSegUtilsError, match="no column '%s'" % name):
            utils.renderColourTable(seg, cols)
    with pytest.raises(utils.PyShepSegUtilsError, match='outside 0..255'):
        utils.renderColourTable(seg, four(5, Green=np.array([0, 1, 2, 3, 256])))
    with pytest.raises(utils.PyShepSegUtilsError, match='integer array'):
        utils.renderColourTable(seg, four(5, Blue=np.zeros(5)))
    with pytest.raises(utils.PyShepSegUtilsError, match='ColourTableResult or a mapping'):
        utils.renderColourTable(seg, [1, 2, 3])
    with pytest.raises(utils.PyShepSegUtilsError, match='2-D uint32'):
        utils.renderColourTable(seg.astype(np.int32), four(5))
    with pytest.raises(utils.PyShepSegUtilsError, match='2-D uint32'):
        utils.renderColourTable(seg[0], four(5))
    with pytest.raises(utils.PyShepSegUtilsError, match='.npy path'):
        utils.renderColourTable(seg, four(5), outfile='out.tif')
    assert asked == []


def test_no_cpu_fallback_without_gpu():
    from pyshepseg_amd import _lib, utils
    if _lib.lib().shp_device_count() > 0:
        pytest.skip('a GPU is present')
    cols = {'a': np.arange(5.0), 'b': np.arange(5.0), 'c': np.arange(5.0)}
    with pytest.raises(_lib.ShepsegHipError):
        utils.writeColorTableFromRatColumns(cols, 'a', 'b', 'c')
    with pytest.raises(_lib.ShepsegHipError):
        utils.renderColourTable(np.zeros((4, 4), dtype=np.uint32), four(5))


@pytest.mark.parametrize('n', [1, 2, 1000])
def test_random_colour_table_in_memory(n):
    from pyshepseg_amd import utils
    t = utils.writeRandomColourTable(None, n, seed=4)
    assert sorted(t.columns) == ['Alpha', 'Blue', 'Green', 'Red'] and t.stretch is None
    for name in t.columns:
        assert t.columns[name].dtype == np.uint8 and t.columns[name].shape == (n,)
    assert t.columns['Alpha'][0] == 0 and (t.columns['Alpha'][1:] == 255).all()
    same = utils.writeRandomColourTable(None, n, seed=4)
    other = utils.writeRandomColourTable(None, n, seed=5)
    for name in ('Red', 'Green', 'Blue'):
        assert np.array_equal(t.columns[name], same.columns[name])
    if n == 1000:
        for name in ('Red', 'Green', 'Blue'):
            assert not np.array_equal(t.columns[name], other.columns[name])
            assert t.columns[name].min() < 8 and t.columns[name].max() > 247        # the whole range is used
        assert not np.array_equal(t.columns['Red'], t.columns['Green'])
        assert not np.array_equal(utils.writeRandomColourTable(None, n).columns['Red'],
                                  utils.writeRandomColourTable(None, n).columns['Red'])     # unseeded: fresh entropy
    with pytest.raises(utils.PyShepSegUtilsError):
        utils.writeRandomColourTable(None, 0)


def test_random_colour_table_through_gdal(gdal):  # noqa: F811
    """the columns are created Integer with GDAL's four colour usages in the reference's order (utils.py:139-159),
    found again by usage on a second call -- under whatever name -- and not duplicated"""
    from pyshepseg_amd import utils
    segds = make_image(gdal, 'seg.kea', np.zeros((1, 4, 4), dtype=np.uint32), 0)
    band = segds.GetRasterBand(1)
    rat = band.GetDefaultRAT()
    rat.CreateColumn('Histogram', gdal.GFT_Real, gdal.GFU_PixelCount)
    del gdal.CALLS[:]
    t = utils.writeRandomColourTable(band, 50, seed=1)
    created = [c for c in gdal.CALLS if c[0] == 'RAT.CreateColumn']
    assert created == [('RAT.CreateColumn', 'Blue', 0, 8), ('RAT.CreateColumn', 'Green', 0, 7),
                       ('RAT.CreateColumn', 'Red', 0, 6), ('RAT.CreateColumn', 'Alpha', 0, 9)]
    assert ('RAT.SetRowCount', 50) in gdal.CALLS and rat.GetRowCount() == 50
    names = [rat.GetNameOfCol(i) for i in range(rat.GetColumnCount())]
    assert names == ['Histogram', 'Blue', 'Green', 'Red', 'Alpha']
    for name in ('Red', 'Green', 'Blue', 'Alpha'):
        i = names.index(name)
        assert rat.GetTypeOfCol(i) == gdal.GFT_Integer
        assert np.array_equal(rat.ReadAsArray(i), t.columns[name].astype(np.int64))
    del gdal.CALLS[:]
    t2 = utils.writeRandomColourTable(band, 50, seed=2)
    assert not [c for c in gdal.CALLS if c[0] == 'RAT.CreateColumn'] and rat.GetColumnCount() == 5
    assert np.array_equal(rat.ReadAsArray(names.index('Red')), t2.columns['Red'].astype(np.int64))
    assert not np.array_equal(t.columns['Red'], t2.columns['Red'])
    # a table whose colour columns carry other names: the usage decides
    other = make_image(gdal, 'other.kea', np.zeros((1, 4, 4), dtype=np.uint32), 0).GetRasterBand(1)
    orat = other.GetDefaultRAT()
    orat.CreateColumn('rouge', gdal.GFT_Integer, 6)
    del gdal.CALLS[:]
    t3 = utils.writeRandomColourTable(other, 7, seed=3)
    assert [c[1] for c in gdal.CALLS if c[0] == 'RAT.CreateColumn'] == ['Blue', 'Green', 'Alpha']
    assert np.array_equal(orat.ReadAsArray(0), t3.columns['Red'].astype(np.int64))
