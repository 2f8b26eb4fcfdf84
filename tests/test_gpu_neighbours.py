"""GPU: neighbours.findSegmentNeighbours against the numpy definition (tests/neighbour_cases.py), array for array with
numpy.array_equal: everything is integer, nothing has a tolerance.  The kernel counts the pairs of 32 x 64 patches
in an LDS hash table, so the shapes below are chosen by where that can go wrong: pairs across patch edges and
corners, patches whose pairs do not fit the table, one pair or one segment that is everywhere, ids far apart."""
import ctypes
import functools
import os

import numpy as np
import pytest

import neighbour_cases as nc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize('four', [True, False], ids=['4conn', '8conn'])


def find(seg, four=True, **kw):
    from pyshepseg_amd import neighbours
    return neighbours.findSegmentNeighbours(seg, fourConnected=four, **kw)


def assert_table(got, want, four=None):
    (offsets, nbrs, lens) = want
    assert got.offsets.dtype == np.int64 and got.neighbours.dtype == np.uint32 and got.borderLengths.dtype == np.int64
    assert got.maxSegId == len(offsets) - 2
    assert np.array_equal(got.offsets, offsets)
    assert np.array_equal(got.neighbours, nbrs)
    assert np.array_equal(got.borderLengths, lens)
    assert 2 * got.pairsSeen == int(lens.sum())
    assert len(nbrs) // 2 <= got.recordsSorted <= got.pairsSeen
    if four is not None:
        assert got.fourConnected is four


def check(seg, four, maxSegId=None, **kw):
    got = find(seg, four, maxSegId=maxSegId, **kw)
    assert_table(got, nc.reference_neighbours(seg, four, maxSegId), four)
    return got


@functools.lru_cache(maxsize=None)
def real_raster(name):
    if name == 'mosaic':
        with np.load(os.path.join(GOLDEN, 'ci_scenario_1000.npz')) as z:
            seg = z['mosaic']
    elif name == 'random1024':
        seg = nc.random_labels((1024, 1024), 39999, 1)
    else:
        with np.load(os.path.join(GOLDEN, 'tile_synth128_null.npz')) as z:
            seg = z[name]
    seg = np.ascontiguousarray(seg, dtype=np.uint32)
    seg.setflags(write=False)
    return seg


@functools.lru_cache(maxsize=None)
def real_reference(name, four):
    return nc.reference_neighbours(real_raster(name), four)


# ---- 1: the worked example ----------------------------------------------------------------------------------
@BOTH
def test_example(four):
    got = find(nc.EXAMPLE, four)
    assert got.offsets.tolist() == nc.EXAMPLE_OFFSETS
    assert got.neighbours.tolist() == nc.EXAMPLE_NEIGHBOURS
    assert got.borderLengths.tolist() == nc.EXAMPLE_LENGTHS[four]
    assert got.maxSegId == 3 and got.fourConnected is four
    cols = got.columns
    assert cols['numNeighbours'].tolist() == [0, 2, 2, 2]
    assert cols['borderLength'].tolist() == [0, sum(nc.EXAMPLE_LENGTHS[four][0:2]), sum(nc.EXAMPLE_LENGTHS[four][2:4]),
                                             sum(nc.EXAMPLE_LENGTHS[four][4:6])]
    (ids, lens) = got.neighboursOf(2)
    assert ids.tolist() == [1, 3] and lens.tolist() == nc.EXAMPLE_LENGTHS[four][2:4]
    assert got.deviceMs > 0 and got.timings['total'] > 0


# ---- 2: shapes off the patch grid, degenerate shapes --------------------------------------------------------
@BOTH
@pytest.mark.parametrize('top', [5, 3000])
@pytest.mark.parametrize('shape', nc.OFF_GRID_SHAPES, ids=lambda s: '%dx%d' % s)
def test_shapes_off_the_patch_grid(shape, top, four):
    """pairs across patch edges and corners, the SW diagonal across a patch's left edge included"""
    check(nc.random_labels(shape, top, 7 + shape[0] + top), four)


# ---- 3: more distinct pairs than a patch's table holds ------------------------------------------------------
@BOTH
def test_every_pixel_its_own_segment(four):
    """~4000 / ~8000 distinct pairs per patch: the overflow route"""
    got = check(nc.every_pixel_its_own(), four)
    if not four:
        assert len(got.neighbours) == 71604 and int(got.columns['numNeighbours'].max()) == 8


# ---- 4: counts that add up over many patches ----------------------------------------------------------------
@BOTH
def test_half_planes(four):
    got = check(nc.half_planes(), four)
    assert got.borderLengths.tolist() == ([300, 300] if four else [898, 898])


@BOTH
def test_stripes(four):
    """one pair in every lane of every row: it must be counted once per run, and comes out of each patch as one record"""
    got = check(nc.stripes(), four)
    assert got.neighbours.tolist() == [2, 1]
    assert got.recordsSorted * 100 < got.pairsSeen


# ---- 5: one hot segment --------------------------------------------------------------------------------------
@BOTH
def test_one_hot_segment(four):
    got = check(nc.hot_segment(), four)
    assert len(got.neighboursOf(1)[0]) == 150 * 150


# ---- 6: sparse ids -------------------------------------------------------------------------------------------
@BOTH
def test_sparse_ids(four):
    got = check(nc.sparse_ids(), four, maxSegId=nc.SPARSE_MAX)
    assert len(got.offsets) == nc.SPARSE_MAX + 2
    assert len(got.neighboursOf(6)[0]) == 0 and len(got.neighboursOf(nc.SPARSE_MAX)[0]) == 0
    # without maxSegId the table ends at the largest label, found on the GPU
    assert find(nc.sparse_ids(), four).maxSegId == 1 << 20


# ---- 7: zeros ------------------------------------------------------------------------------------------------
@BOTH
def test_zeros(four):
    got = check(np.zeros((70, 130), dtype=np.uint32), four)
    assert got.offsets.tolist() == [0, 0] and len(got.neighbours) == 0 and len(got.borderLengths) == 0
    got = check(np.zeros((70, 130), dtype=np.uint32), four, maxSegId=9)
    assert got.offsets.tolist() == [0] * 11
    got = check(nc.enclosed_by_zeros(), four)
    assert got.columns['numNeighbours'].tolist() == [0, 1, 1, 0]
    for shape in ((0, 5), (5, 0), (0, 0)):
        got = find(np.zeros(shape, dtype=np.uint32), four, maxSegId=4)
        assert got.offsets.tolist() == [0] * 6 and len(got.neighbours) == 0 and len(got.borderLengths) == 0
        assert find(np.zeros(shape, dtype=np.uint32), four).offsets.tolist() == [0, 0]


# ---- 8, 9: real label rasters, uniform random labels ----------------------------------------------------------
@BOTH
@pytest.mark.parametrize('name', ['clump', 'seg_final', 'mosaic'])
def test_real_label_rasters(name, four):
    assert_table(find(real_raster(name), four), real_reference(name, four), four)


def test_random_1024():
    got = find(real_raster('random1024'), False)
    assert len(got.neighbours) == 8352378
    assert_table(got, real_reference('random1024', False), False)


# ---- 10: the table does not depend on the row blocks ---------------------------------------------------------
@pytest.mark.parametrize('rows', [1, 7, 33])
@pytest.mark.parametrize('name,four', [('clump', True), ('clump', False), ('seg_final', True), ('seg_final', False),
                                       ('mosaic', True), ('mosaic', False), ('random1024', False)])
def test_block_independence(name, four, rows):
    seg = real_raster(name)
    got = find(seg, four, chunkPixels=rows * seg.shape[1])
    want = real_reference(name, four)
    assert got.offsets.tobytes() == want[0].tobytes()
    assert got.neighbours.tobytes() == want[1].tobytes()
    assert got.borderLengths.tobytes() == want[2].tobytes()
    assert 2 * got.pairsSeen == int(want[2].sum())


@BOTH
def test_npy_path_and_result_object(four, tmp_path):
    from pyshepseg_amd import tiling
    seg = real_raster('mosaic')
    path = str(tmp_path / 'labels.npy')
    np.save(path, seg)
    want = real_reference('mosaic', four)
    assert_table(find(path, four), want, four)
    assert_table(find(path, four, chunkPixels=33 * seg.shape[1]), want, four)
    res = tiling.TiledSegmentationResult()
    res.segimg = seg
    assert_table(find(res, four, chunkPixels=7 * seg.shape[1]), want, four)


def test_device_resident_labels():
    """labels kept in HBM by the tiled segmentation, read in place: whole and in row blocks, against the table of
    their downloaded copy"""
    from pyshepseg_amd import _lib, tiling
    ras = tiling.DeviceRaster.synth(3, 3, 300, 902)
    try:
        cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=3)
        rd = tiling.doTiledShepherdSegmentation(ras, tiling._KEEP_ON_DEVICE, tileSize=256, overlapSize=64,
                                                minSegmentSize=30, numClusters=12, fixedKMeansInit=True,
                                                concurrencyCfg=cfg)
        try:
            got = {(four, rows): find(rd, four, chunkPixels=None if rows is None else 902 * rows)
                   for four in (True, False) for rows in (None, 1, 7, 33)}
            segimg = np.empty((300, 902), dtype=np.uint32)
            c = _lib.ctx()
            c.check(c._L.shp_dev_download(c.handle, segimg.ctypes.data_as(ctypes.c_void_p),
                                          ctypes.c_void_p(rd.outDev[0]), segimg.nbytes))
            maxSegId = rd.maxSegId
        finally:
            tiling.freeDeviceOutput(rd)
    finally:
        ras.free()
    assert int(segimg.max()) == maxSegId
    for four in (True, False):
        want = nc.reference_neighbours(segimg, four)
        for rows in (None, 1, 7, 33):
            assert_table(got[(four, rows)], want, four)
        assert_table(find(segimg, four), want, four)


# ---- 11: a label above maxSegId ------------------------------------------------------------------------------
@BOTH
def test_label_above_max_seg_id(four):
    from pyshepseg_amd import neighbours
    seg = np.array(real_raster('seg_final'))
    top = int(seg.max())
    with pytest.raises(neighbours.PyShepSegNeighboursError, match='segment id %d is above maxSegId %d' % (top, top - 1)):
        find(seg, four, maxSegId=top - 1)
    # the largest of several, wherever it lies, also inside a uniform area that has no differing pair
    seg[5:9, 5:9] = top + 7
    seg[127, 127] = 0xFFFFFFF0
    seg[64, 0] = top + 100
    with pytest.raises(neighbours.PyShepSegNeighboursError, match='segment id %d is above maxSegId %d' % (0xFFFFFFF0, top)):
        find(seg, four, maxSegId=top, chunkPixels=7 * 128)
    solid = np.full((40, 70), 9, dtype=np.uint32)
    with pytest.raises(neighbours.PyShepSegNeighboursError, match='segment id 9 is above maxSegId 8'):
        find(solid, four, maxSegId=8)
    assert_table(find(solid, four, maxSegId=9), nc.reference_neighbours(solid, four, 9), four)
