"""GPU: neighbours.mergeSegments against its definition in numpy (tests/merge_cases.py).  Everything is an integer and
compared with numpy.array_equal; the contracted table is also compared with the neighbour table of the recoded
raster, built on the GPU (the round trip)."""
import ctypes
import functools

import numpy as np
import pytest

import merge_cases as mc
import neighbour_cases as nc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def built(name, four):
    """(seg, S, keys, segSize or None, the model's result): computed once, shared, left unchanged"""
    case = [c for c in mc.CASES if c.name == name][0]
    (seg, S, keys, size, table) = mc.build(case, four)
    model = mc.reference_merge(table, keys, case.ignoreKey, case.minBorder, size)
    model.rasterTable = mc.raster_route(seg, four, model)
    return (case, seg, S, keys, size, model)


def assert_table(nb, want, M, what=''):
    assert nb.maxSegId == M, what
    for (got, exp, name) in zip((nb.offsets, nb.neighbours, nb.borderLengths), want, ('offsets', 'neighbours', 'lengths')):
        assert got.dtype == exp.dtype and np.array_equal(got, exp), (what, name)


def assert_groups(res, model):
    assert res.maxSegId == model.maxSegId
    for name in ('recode', 'representative', 'groupSize'):
        (got, exp) = (getattr(res, name), getattr(model, name))
        assert got.dtype == exp.dtype and np.array_equal(got, exp), name
    assert (res.links, res.recordsSorted) == (model.links, model.recordsSorted)
    assert_table(res.neighbours, model.table, model.maxSegId, 'graph route')
    assert res.neighbours.recordsSorted == model.recordsSorted


@pytest.mark.parametrize('four', [True, False])
@pytest.mark.parametrize('case', mc.CASES, ids=repr)
def test_case_equals_model(case, four):
    """cases a to i: the groups, the contracted table by both routes, the recoded raster and its histogram"""
    from pyshepseg_amd import neighbours
    (case, seg, S, keys, size, model) = built(case.name, four)
    nb = neighbours.findSegmentNeighbours(seg, four, maxSegId=S)
    res = neighbours.mergeSegments(nb, keys, ignoreKey=case.ignoreKey, minBorder=case.minBorder, segSize=size, segfile=seg)
    assert_groups(res, model)
    assert_table(res.neighbours, model.rasterTable, model.maxSegId, 'raster route')
    assert res.neighbours.fourConnected == four and res.neighbours.residentSerial == neighbours.residentTableSerial()
    assert res.segimg.dtype == np.uint32 and np.array_equal(res.segimg, model.recode[seg])
    hist = np.bincount(model.recode[seg].ravel(), minlength=model.maxSegId + 1)
    assert res.hist.dtype == np.int64 and np.array_equal(res.hist, hist)
    if size is not None:
        assert np.array_equal(res.hist, model.hist)
    assert res.outDev is None and res.deviceMs > 0


def test_example_by_hand():
    from pyshepseg_amd import neighbours
    for (keys, answer) in ((mc.EXAMPLE_KEYS_A, mc.EXAMPLE_ANSWER_A), (mc.EXAMPLE_KEYS_B, mc.EXAMPLE_ANSWER_B)):
        for four in (True, False):
            nb = neighbours.findSegmentNeighbours(nc.EXAMPLE, four)
            res = neighbours.mergeSegments(nb, keys, segSize=np.bincount(nc.EXAMPLE.ravel()))
            assert res.recode.tolist() == answer['recode'] and res.maxSegId == answer['maxSegId']
            assert res.representative.tolist() == answer['representative']
            assert res.groupSize.tolist() == answer['groupSize'] and res.hist.tolist() == answer['hist']
            assert (res.links, res.recordsSorted) == (answer['links'], answer['recordsSorted'])
            assert res.neighbours.offsets.tolist() == answer['offsets']
            assert res.neighbours.neighbours.tolist() == answer['neighbours']
            assert res.neighbours.borderLengths.tolist() == answer['lengths'][four]
            assert res.segimg is None and res.outDev is None
            assert neighbours.mergeSegments(nb, keys).hist is None


@pytest.mark.parametrize('four', [True, False])
def test_min_border_is_a_threshold(four):
    """the half planes merge at their border length and not one above it"""
    from pyshepseg_amd import neighbours
    nb = neighbours.findSegmentNeighbours(nc.half_planes(), four)
    border = mc.HALF_PLANES_BORDER[four]
    assert nb.borderLengths.tolist() == [border, border]
    at = neighbours.mergeSegments(nb, np.zeros(3, dtype=np.int8), minBorder=border)
    assert (at.maxSegId, at.links, at.recordsSorted, len(at.neighbours.neighbours)) == (1, 1, 0, 0)
    above = neighbours.mergeSegments(nb, np.zeros(3, dtype=np.int8), minBorder=border + 1)
    assert (above.maxSegId, above.links, above.recordsSorted) == (2, 0, 1)
    assert above.neighbours.borderLengths.tolist() == [border, border]


def test_hand_built_table_equals_resident():
    """case j: a table built by hand is uploaded and gives what the resident one gives; the contracted table is then
    the resident one, the old one is not"""
    from pyshepseg_amd import neighbours
    (case, seg, S, keys, size, model) = built('drawn_large', True)
    nb = neighbours.findSegmentNeighbours(seg, True, maxSegId=S)
    resident = neighbours.mergeSegments(nb, keys)
    assert resident.timings['uploaded'] is False
    byHand = neighbours.SegmentNeighbours(nb.offsets.copy(), nb.neighbours.copy(), nb.borderLengths.copy(), S, True)
    res = neighbours.mergeSegments(byHand, keys)
    assert res.timings['uploaded'] is True
    assert_groups(res, model)
    assert_groups(resident, model)
    column = np.arange(res.maxSegId + 1, dtype=np.float64)
    out = neighbours.reduceOverNeighbours(res.neighbours, [(column, [('n', 'count')])])
    assert res.neighbours.reduceTimings['uploaded'] is False
    assert np.array_equal(out['n'], np.diff(model.table[0]))
    out = neighbours.reduceOverNeighbours(nb, [(np.arange(S + 1, dtype=np.float64), [('n', 'count')])])
    assert nb.reduceTimings['uploaded'] is True
    assert np.array_equal(out['n'], np.diff(nb.offsets))
    # the first result's table has been displaced by then and is uploaded again as well
    out = neighbours.reduceOverNeighbours(resident.neighbours, [(column, [('n', 'count')])])
    assert resident.neighbours.reduceTimings['uploaded'] is True and np.array_equal(out['n'], np.diff(model.table[0]))


def _round_trip(res, output, four):
    from pyshepseg_amd import neighbours
    again = neighbours.findSegmentNeighbours(output, four, maxSegId=res.maxSegId)
    assert_table(again, (res.neighbours.offsets, res.neighbours.neighbours, res.neighbours.borderLengths), res.maxSegId,
                 'round trip')


@pytest.mark.parametrize('four', [True, False])
@pytest.mark.parametrize('name,rows', [('drawn_small', None), ('drawn_tiny', 11), ('drawn_small', 17), ('drawn_large', 60)])
def test_raster_array_and_file(name, rows, four, tmp_path):
    """case k: an array with the default blocks, and .npy files in three to five row blocks ((33, 65) in blocks of 11
    rows; (65, 129) in blocks of 17 has a last block of 14; (257, 300) in blocks of 60 one of 17), with the histogram
    counted in the pass"""
    from pyshepseg_amd import neighbours
    (case, seg, S, keys, size, model) = built(name, four)
    want = model.recode[seg]
    hist = np.bincount(want.ravel(), minlength=model.maxSegId + 1)
    nb = neighbours.findSegmentNeighbours(seg, four, maxSegId=S)
    if rows is None:
        res = neighbours.mergeSegments(nb, keys, segfile=seg)
        output = res.segimg
    else:
        (src, dst) = (str(tmp_path / 'seg.npy'), str(tmp_path / 'merged.npy'))
        np.save(src, seg)
        assert -(-seg.shape[0] // rows) >= 3
        res = neighbours.mergeSegments(nb, keys, segfile=src, outfile=dst, chunkPixels=rows * seg.shape[1])
        assert res.segimg is None and res.outDev is None
        output = np.load(dst)
    assert output.dtype == np.uint32 and np.array_equal(output, want)
    assert np.array_equal(res.hist, hist)
    assert_groups(res, model)
    _round_trip(res, output, four)
    if rows is not None:
        # an array into a file, and the sized merge leaves the histogram to segSize
        sized = neighbours.mergeSegments(nb, keys, segSize=np.bincount(seg.ravel(), minlength=S + 1), segfile=seg,
                                         outfile=dst, chunkPixels=rows * seg.shape[1])
        assert sized.segimg is None and np.array_equal(np.load(dst), want) and np.array_equal(sized.hist, hist)


def test_device_resident_labels():
    """case k: the labels the tiled segmentation kept in HBM are recoded into a second device raster, which
    findSegmentNeighbours reads in place"""
    from pyshepseg_amd import _lib, tiling, neighbours
    (nrows, ncols) = (300, 902)
    ras = tiling.DeviceRaster.synth(3, 3, nrows, ncols)
    try:
        cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=3)
        rd = tiling.doTiledShepherdSegmentation(ras, tiling._KEEP_ON_DEVICE, tileSize=256, overlapSize=64,
                                                minSegmentSize=30, numClusters=12, fixedKMeansInit=True,
                                                concurrencyCfg=cfg)
        res = None
        try:
            c = _lib.ctx()

            def download(outDev):
                img = np.empty((nrows, ncols), dtype=np.uint32)
                c.check(c._L.shp_dev_download(c.handle, img.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(outDev[0]),
                                              img.nbytes))
                return img

            seg = download(rd.outDev)
            S = rd.maxSegId
            keys = (np.arange(S + 1) % 3).astype(np.int32)
            for (four, rows) in ((True, None), (False, 7)):
                nb = neighbours.findSegmentNeighbours(rd, four, maxSegId=S)
                res = neighbours.mergeSegments(nb, keys, segfile=rd, chunkPixels=None if rows is None else rows * ncols)
                model = mc.reference_merge(nc.reference_neighbours(seg, four, S), keys)
                assert_groups(res, model)
                assert res.segimg is None and res.outDev[1:3] == (nrows, ncols) and res.outDev[0] != rd.outDev[0]
                assert np.array_equal(download(rd.outDev), seg)                 # (not in place)
                assert np.array_equal(download(res.outDev), model.recode[seg])
                assert np.array_equal(res.hist, np.bincount(model.recode[seg].ravel(), minlength=model.maxSegId + 1))
                _round_trip(res, res, four)
                tiling.freeDeviceOutput(res)
                res = None
        finally:
            if res is not None:
                tiling.freeDeviceOutput(res)
            tiling.freeDeviceOutput(rd)
    finally:
        ras.free()


def test_label_above_the_table_raises(tmp_path):
    """a raster with labels the table has no rows for: the largest one is named, whatever block it lies in, and
    nothing is read past the recode array"""
    from pyshepseg_amd import neighbours
    (case, seg, S, keys, size, model) = built('drawn_small', True)
    nb = neighbours.findSegmentNeighbours(seg, True, maxSegId=S)
    bad = seg.copy()
    bad[3, 5] = S + 7
    bad[40, 100] = 0xFFFFFFF0
    bad[64, 128] = S + 1
    with pytest.raises(neighbours.PyShepSegNeighboursError, match='segment id {} is above maxSegId {}'.format(0xFFFFFFF0, S)):
        neighbours.mergeSegments(nb, keys, segfile=bad)
    with pytest.raises(neighbours.PyShepSegNeighboursError, match='segment id {} is above maxSegId {}'.format(0xFFFFFFF0, S)):
        neighbours.mergeSegments(nb, keys, segfile=bad, outfile=str(tmp_path / 'out.npy'), chunkPixels=17 * seg.shape[1])
    # the groups do not depend on the raster: the same call with the raster they came from still works
    assert_groups(neighbours.mergeSegments(nb, keys, segfile=seg), model)


@pytest.mark.parametrize('segOffset,outOffset', [(0, 0), (0, 1), (1, 1), (1, 0), (2, 3), (3, 2)])
def test_recode_call_at_every_alignment(segOffset, outOffset):
    """shp_nbr_merge_recode_dev with labels and output at offsets of whole words from a 16-byte boundary: the Python
    layer gives the output the labels' offset, where the kernel stores whole vectors; any other pair of offsets takes
    its word-by-word stores, and a label offset its one-by-one head"""
    from pyshepseg_amd import _lib, neighbours
    (case, seg, S, keys, size, model) = built('drawn_small', True)
    nb = neighbours.findSegmentNeighbours(seg, True, maxSegId=S)
    res = neighbours.mergeSegments(nb, keys)
    assert np.array_equal(res.recode, model.recode)
    c = _lib.ctx()
    L = c._L
    labels = np.ascontiguousarray(seg.ravel()[:8001])           # (with labels left over behind the last group of four)
    n = labels.size
    want = model.recode[labels]
    (dSeg, dOut) = (ctypes.c_void_p(), ctypes.c_void_p())
    try:
        c.check(L.shp_dev_alloc(c.handle, n * 4 + 16, ctypes.byref(dSeg)))
        c.check(L.shp_dev_alloc(c.handle, n * 4 + 16, ctypes.byref(dOut)))
        assert dSeg.value % 16 == 0 and dOut.value % 16 == 0
        (pSeg, pOut) = (ctypes.c_void_p(dSeg.value + 4 * segOffset), ctypes.c_void_p(dOut.value + 4 * outOffset))
        c.check(L.shp_dev_upload(c.handle, pSeg, _lib.ptr(labels), labels.nbytes))
        for count in (1, 0):
            (bad, ms) = (ctypes.c_uint32(0), ctypes.c_double(0))
            c.check(L.shp_nbr_merge_recode_dev(c.handle, pSeg, n, pOut, count, ctypes.byref(bad), ctypes.byref(ms)))
            got = np.zeros(n, dtype=np.uint32)
            c.check(L.shp_dev_download(c.handle, _lib.ptr(got), pOut, got.nbytes))
            assert bad.value == 0 and np.array_equal(got, want)
        hist = np.empty(model.maxSegId + 1, dtype=np.int64)
        c.check(L.shp_nbr_merge_groups(c.handle, None, None, None, _lib.ptr(hist)))
        assert np.array_equal(hist, np.bincount(want, minlength=model.maxSegId + 1))
    finally:
        for p in (dSeg, dOut):
            if p.value:
                c.check(L.shp_dev_free(c.handle, p))
