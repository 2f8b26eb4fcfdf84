"""CPU: the host side of the colour table and the RGBA rendering on the row-sharded multi-rank output
(distributed.colourShares, statsColumnsByName, _NpyRgbaPatchWriter, and the argument errors of
writeColorTableFromRatColumnsDistributed / renderColourTableDistributed that are raised before any device work)."""
import os

import numpy as np
import pytest


def test_share_plan_covers_the_rows_once_in_order():
    """worlds 1-8, columns from one row (fewer rows than ranks: empty shares) to a few thousand: the shares are
    consecutive, in rank order, cover 0..n-1 once, differ by at most one row, and are the statistics' idRange"""
    from pyshepseg_amd import distributed
    for world in range(1, 9):
        for n in list(range(1, 20)) + [97, 1000, 4099]:
            shares = distributed.colourShares(n, world)
            assert len(shares) == world
            assert shares == [distributed.idRange(r, world, n - 1) for r in range(world)]
            assert shares[0][0] == 0 and shares[-1][1] == n
            for ((_a, b), (a2, _b2)) in zip(shares, shares[1:]):
                assert b == a2
            sizes = [b - a for (a, b) in shares]
            assert min(sizes) >= 0 and max(sizes) - min(sizes) <= 1
            assert [i for (a, b) in shares for i in range(a, b)] == list(range(n))
            if n < world:
                assert sizes.count(0) == world - n


def test_rgba_patch_writer_round_trip(tmp_path):
    """rectangles and whole rows written through _NpyRgbaPatchWriter == the same stores into a numpy array; a file
    of another shape or dtype, and a rectangle that leaves the raster, are refused"""
    from pyshepseg_amd import distributed, tiling
    rng = np.random.default_rng(3)
    (nr, nc) = (37, 29)
    path = str(tmp_path / 'rgba.npy')
    tiling._NpyRowWriter(path, nr, nc, dtype=np.uint8, pixelShape=(4,)).close()
    assert np.array_equal(np.load(path), np.zeros((nr, nc, 4), dtype=np.uint8))
    want = np.zeros((nr, nc, 4), dtype=np.uint8)
    w = distributed._NpyRgbaPatchWriter(path, nr, nc)
    try:
        for (y0, x0, h, wd) in [(0, 0, 5, nc), (5, 3, 7, 11), (30, 0, 7, nc), (12, 28, 20, 1), (11, 0, 1, 1),
                                (6, 10, 3, 19)]:
            v = rng.integers(0, 256, size=(h, wd, 4), dtype=np.uint8)
            w.writeRect(y0, x0, v)
            want[y0:y0 + h, x0:x0 + wd] = v
        big = rng.integers(0, 256, size=(9, nc + 6, 4), dtype=np.uint8)
        w.writeRect(20, 2, big[:, 4:14])                          # a view that is not contiguous
        want[20:29, 2:12] = big[:, 4:14]
        with pytest.raises(tiling.PyShepSegTilingError):
            w.writeRect(35, 0, np.zeros((3, nc, 4), dtype=np.uint8))
        with pytest.raises(tiling.PyShepSegTilingError):
            w.writeRect(0, 0, np.zeros((3, nc), dtype=np.uint32))
    finally:
        w.close()
    got = np.load(path)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    labels = str(tmp_path / 'labels.npy')
    tiling._NpyRowWriter(labels, nr, nc).close()
    for (p, shape) in [(labels, (nr, nc)), (path, (nr, nc + 1)), (path, (nr + 1, nc))]:
        with pytest.raises(tiling.PyShepSegTilingError):
            distributed._NpyRgbaPatchWriter(p, *shape)
    with pytest.raises(tiling.PyShepSegTilingError):
        distributed._NpyPatchWriter(path, nr, nc)                 # (and the uint32 writer refuses the RGBA file)


def test_stats_columns_by_name():
    """int and float columns land under their names by the fast selection, for several entries and for one"""
    from pyshepseg_amd import distributed, tilingstats
    entries = [(1, [('m1', 'mean'), ('n1', 'pixcount')]), (3, [('sd3', 'stddev'), ('med3', 'median')]),
               (2, [('min2', 'min'), ('m2', 'mean')])]
    (fast, _b, nInt, nFloat) = tilingstats.makeBandStatsSelection(entries)
    assert (nInt, nFloat) == (3, 3)
    ic = np.arange(nInt * 5, dtype=np.int64).reshape(nInt, 5)
    fc = (100 + np.arange(nFloat * 5, dtype=np.float32)).reshape(nFloat, 5)
    cols = distributed.statsColumnsByName(entries, ic, fc, fast)
    assert list(cols) == ['m1', 'n1', 'sd3', 'med3', 'min2', 'm2']
    want = {'m1': fc[0], 'n1': ic[0], 'sd3': fc[1], 'med3': ic[1], 'min2': ic[2], 'm2': fc[2]}
    for (k, v) in want.items():
        assert cols[k].dtype == v.dtype and np.array_equal(cols[k], v), k
    one = [(2, [('a', 'max'), ('b', 'mean')])]
    (f1, n1, m1) = tilingstats.makeFastStatsSelection([0, 1], one[0][1])
    c1 = distributed.statsColumnsByName(one, ic[:n1], fc[:m1], f1)
    assert np.array_equal(c1['a'], ic[0]) and np.array_equal(c1['b'], fc[0])
    with pytest.raises(tilingstats.PyShepSegStatsError):
        distributed.statsColumnsByName(entries[:2], ic, fc, fast)


def test_overview_holes_are_the_pixels_no_block_writes():
    """overviewHoles against the host simulation of the one-GPU driver's overview writes: the listed columns and
    rows are exactly the layer pixels no tile wrote (geometries with and without holes)"""
    import dist_cases
    import dist_output_helpers as OH
    from pyshepseg_amd import distributed
    seen = 0
    for (nr, nc, tile, ov, levels) in [(300, 260, 100, 20, [2, 4, 16, 32]), (1500, 1300, 512, 128, [2, 4, 8, 16]),
                                       (203, 190, 64, 24, [2, 8, 32])]:
        ti = dist_cases.tileInfoOf(nr, nc, tile, ov)
        mosaic = np.ones((nr, nc), dtype=np.uint32)
        for lvl in levels:
            (_layer, owner) = OH.simulateOverview(mosaic, ti, ov, lvl)
            (cols, rows) = distributed.overviewHoles(ti, ov, lvl)
            want = np.zeros(owner.shape, dtype=bool)
            want[:, cols] = True
            want[rows, :] = True
            assert np.array_equal(want, owner < 0), (nr, nc, lvl)
            seen += int(want.any())
    assert seen >= 2


class _HostEngine(object):
    """an engine without the device methods"""


class _Dres(object):
    (nRows, nCols, outRows, maxSegId) = (10, 10, (0, 10), 4)


def test_engine_without_device_methods():
    from pyshepseg_amd import comm, distributed, utils
    cols = {'r': np.arange(5.0), 'g': np.arange(5.0), 'b': np.arange(5.0)}
    with pytest.raises(utils.PyShepSegUtilsError, match=r'needs a device engine \(HipEngine\)'):
        distributed.writeColorTableFromRatColumnsDistributed(_HostEngine(), comm.LocalComm(), cols, 'r', 'g', 'b')
    with pytest.raises(utils.PyShepSegUtilsError, match=r'needs a device engine \(HipEngine\)'):
        distributed.renderColourTableDistributed(_HostEngine(), comm.LocalComm(), _Dres(),
                                                 colours=utils.writeRandomColourTable(None, 5, seed=1))


class _NoDeviceEngine(object):
    """has the methods, must never reach them"""
    colourTable = None

    def colourTableOnDevice(self, *a, **k):
        raise AssertionError('device work before the argument check')

    renderOnDevice = colourTableOnDevice


def test_argument_errors_before_device_work():
    from pyshepseg_amd import comm, distributed, utils
    cols = {'r': np.arange(5.0), 'g': np.arange(5.0)}
    with pytest.raises(utils.PyShepSegUtilsError, match="column 'b' is not in the table"):
        distributed.writeColorTableFromRatColumnsDistributed(_NoDeviceEngine(), comm.LocalComm(), cols, 'r', 'g', 'b')
    with pytest.raises(utils.PyShepSegUtilsError, match='holds no colour table'):
        distributed.renderColourTableDistributed(_NoDeviceEngine(), comm.LocalComm(), _Dres())
    with pytest.raises(utils.PyShepSegUtilsError, match="no column 'Alpha'"):
        distributed.renderColourTableDistributed(_NoDeviceEngine(), comm.LocalComm(), _Dres(),
                                                 colours={'Red': [1], 'Green': [1], 'Blue': [1]})


def test_bad_outfile_is_refused_before_anything_is_created(tmp_path):
    from pyshepseg_amd import comm, distributed, tiling, utils
    table = utils.writeRandomColourTable(None, 5, seed=1)
    for bad in [str(tmp_path / 'rgba.kea'), str(tmp_path / 'missing' / 'rgba.npy'), 7]:
        with pytest.raises(tiling.PyShepSegTilingError):
            distributed.renderColourTableDistributed(_NoDeviceEngine(), comm.LocalComm(), _Dres(), colours=table,
                                                     outfile=bad)
    assert os.listdir(str(tmp_path)) == []
