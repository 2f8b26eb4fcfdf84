"""GPU: outlines.traceSegmentOutlines against the sequential model (tests/outline_cases.py), numpy.array_equal on every
array, dtype included: everything is integer, nothing has a tolerance.

The kernels (csrc/outline.h) take a pixel, an edge, a ring, a vertex or an id per thread, in workgroups of B = 256
threads (OL_BLOCK), without LDS tiles; the shared scan (csrc/scan.h) takes SCAN_ITEMS = 8192 items a workgroup and the
shared sort (csrc/sort.h) SORT_TILE = 2048 rings.  So the shapes are chosen by counts, not by patches: rasters with 255,
256 and 257 pixels, with 8191, 8192 and 8193; rasters of distinct one-pixel ids, which have four edges, one ring and
four vertices a pixel, with 63, 64 and 65 pixels (256 edges, a workgroup of them), 255 .. 257 (the rings a workgroup
takes), 2047 .. 2049 (8192 edges, a scan block; 2048 rings, a sort tile).  The kernel that finds the sides runs at
most G = 4096 workgroups (OL_MASK_GRID), which stride over larger rasters: G B - 1024, G B and G B + 1024 pixels.  The
doubling rounds are held to ring lengths on both sides of every power of two up to 2^13, and to one ring of more than
2^17 edges.

Not covered: rasters of 2^31 pixels and more (8.6 GB of labels and a model walk of hours)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import neighbour_cases as nc
import outline_cases as oc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ARRAYS = ('ringOffsets', 'vertexOffsets', 'vertices', 'ringArea2')


def trace(seg, **kw):
    from pyshepseg_amd import outlines
    return outlines.traceSegmentOutlines(seg, **kw)


def round_bound(edges):
    """ceil(log2(edges)) + 2"""
    return (max(int(edges), 1) - 1).bit_length() + 2


def assert_same(got, want):
    """want: the model's dictionary, or another SegmentOutlines"""
    if not isinstance(want, dict):
        want = dict({k: getattr(want, k) for k in ARRAYS}, columns=want.columns, maxSegId=want.maxSegId)
    assert got.maxSegId == want['maxSegId']
    for k in ARRAYS:
        a = getattr(got, k)
        assert a.dtype == np.int64 and a.shape == want[k].shape and np.array_equal(a, want[k]), k
    assert sorted(got.columns) == sorted(oc.COLUMNS)
    for k in oc.COLUMNS:
        assert got.columns[k].dtype == np.int64 and np.array_equal(got.columns[k], want['columns'][k]), k
    assert got.rounds <= round_bound(got.edges)


def check(seg, fourConnected=True, maxSegId=None, origin=(0, 0)):
    got = trace(seg, fourConnected=fourConnected, maxSegId=maxSegId, origin=origin)
    assert_same(got, oc.reference_outlines(seg, fourConnected, maxSegId, origin))
    assert got.fourConnected == fourConnected and got.origin == tuple(origin)
    return got


@functools.lru_cache(maxsize=None)
def real_raster(name):
    if name == 'mosaic':
        with np.load(os.path.join(GOLDEN, 'ci_scenario_1000.npz')) as z:
            seg = z['mosaic']
    elif name == 'random1024':
        seg = nc.random_labels((1024, 1024), 39999, 1)
    elif name == 'random256':
        seg = nc.random_labels((256, 256), 2999, 2)
    else:
        with np.load(os.path.join(GOLDEN, 'tile_synth128_null.npz')) as z:
            seg = z[name]
    seg = np.ascontiguousarray(seg, dtype=np.uint32)
    seg.setflags(write=False)
    return seg


@functools.lru_cache(maxsize=None)
def real_model(name, four):
    return oc.reference_outlines(real_raster(name), four)


# ---- both corner rules ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
def test_worked_examples(four):
    got = check(oc.EXAMPLE, four)
    assert got.ringArea2.tolist() == oc.EXAMPLE_AREA2
    assert [r.tolist() for r in got.ringsOf(2)] == [[list(v) for v in oc.EXAMPLE_RINGS[2][0]]]
    assert got.deviceMs > 0 and got.timings['total'] > 0 and got.edges == 24
    got = check(oc.checkerboard(4), four)
    pairs = list(zip(got.ringArea2.tolist(), np.diff(got.vertexOffsets).tolist()))
    assert pairs == ([(2, 4)] * 8 if four else [(20, 24), (-2, 4), (-2, 4)])


@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
@pytest.mark.parametrize('n', [8, 65])
def test_checkerboards(n, four):
    got = check(oc.checkerboard(n), four)
    if four:
        assert got.columns['numParts'][1] == n * n // 2 and got.columns['numHoles'][1] == 0


@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
def test_saddles_in_corners_and_on_rims(four):
    for seg in oc.saddles():
        got = check(seg, four)
        assert got.columns['numParts'][1] == (2 if four else 1)


# ---- ring length against the doubling rounds --------------------------------------------------------------------------
def test_ring_lengths_round_every_power_of_two():
    (lengths, seg) = oc.strips(12)
    assert sorted(set(lengths)) == sorted({2 ** k - d for k in range(1, 13) for d in (0, 1, 2)} - {0})
    got = check(seg)
    assert np.array_equal(oc.ring_lengths(got.vertexOffsets, got.vertices), 2 * np.array(lengths) + 2)
    assert got.rounds == 15 <= round_bound(got.edges)           # 2^13 + 2 edges: 14 rounds to cover them, one to see it
    # each length on its own: the rounds follow the longest ring, one round more than its doubling
    for n in (1, 2, 3, 4, 30, 31, 32):
        one = trace(np.ones((1, n), dtype=np.uint32))
        assert one.rounds == (2 * n + 2 - 1).bit_length() + 1 <= round_bound(one.edges)


def test_one_long_ring():
    seg = oc.serpentine(512)
    got = check(seg)
    r = int(got.ringOffsets[1])
    assert got.ringOffsets[2] - r == 1
    edges = int(oc.ring_lengths(got.vertexOffsets, got.vertices)[r])
    assert edges > 2 ** 17 and got.vertices[got.vertexOffsets[r]].tolist() == [0, 511]
    assert got.rounds == (edges - 1).bit_length() + 1


def test_every_edge_a_turn_edge():
    got = check(oc.staircase())
    r = int(got.ringOffsets[2])
    assert got.vertexOffsets[r + 1] - got.vertexOffsets[r] >= 2 * 69


def test_most_edges_straight():
    for seg in oc.long_strips():
        got = check(seg)
        assert got.vertexOffsets.tolist() == [0, 4] and got.edges == 2 * 4096 + 2


# ---- holes and order --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
def test_holes_and_order(four):
    got = check(oc.concentric_squares(), four)
    assert got.columns['numParts'].tolist() == [0, 3, 2] and got.columns['numHoles'].tolist() == [0, 2, 2]
    assert [len(p) for p in got.polygonsOf(1)] == [2, 2, 1]
    got = check(oc.scattered_parts(), four)
    if four:
        assert got.columns['numParts'][7] == 300 and got.columns['numVertices'][7] == 1200
        first = got.vertices[got.vertexOffsets[got.ringOffsets[7]:got.ringOffsets[8]]]
        keys = first[:, 0] * 1000 + first[:, 1]
        assert np.all(np.diff(keys) > 0)
    got = check(oc.last_pixel_only(), four)
    assert got.ringsOf(5)[0].tolist() == [[36, 69], [36, 70], [37, 70], [37, 69]]


# ---- launch geometry --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1), (1, 65), (65, 1), (1, 255), (1, 256), (257, 1), (16, 16), (1, 8191), (64, 128),
                                   (8193, 1), (33, 65), (91, 90), (129, 65)], ids=lambda s: '%dx%d' % s)
def test_pixel_counts_round_the_workgroup_and_the_scan_block(shape):
    for top in (1, 3, 400):
        check(nc.random_labels(shape, top, shape[0] + 3 * top), top % 2 == 1)


@pytest.mark.parametrize('n', [63, 64, 65, 255, 256, 257, 2047, 2048, 2049])
def test_edge_and_ring_counts_round_the_workgroup_the_scan_block_and_the_sort_tile(n):
    for shape in ((1, n), (n, 1)):
        seg = np.arange(1, n + 1, dtype=np.uint32).reshape(shape)
        got = check(seg)
        assert got.edges == 4 * n and len(got.ringArea2) == n and len(got.vertices) == 4 * n
    # the same rings under a descending numbering: the sort reverses them
    check(np.arange(n, 0, -1, dtype=np.uint32).reshape(1, n))


@pytest.mark.parametrize('rows', [1023, 1024, 1025])
def test_pixel_counts_round_the_side_kernels_grid(rows):
    """G B = 1024 x 1024 pixels; coarse blocks of labels keep the model's walk short"""
    coarse = nc.random_labels((33, 32), 60, rows)
    seg = np.ascontiguousarray(np.kron(coarse, np.ones((32, 32), dtype=np.uint32))[:rows], dtype=np.uint32)
    assert seg.shape == (rows, 1024)
    seg[rows - 1, 1023] = 61                        # the last pixel, of the last stride, has a ring of its own
    got = check(seg, rows % 2 == 1)
    assert got.ringsOf(61)[0].tolist() == [[rows - 1, 1023], [rows - 1, 1024], [rows, 1024], [rows, 1023]]


# ---- ids --------------------------------------------------------------------------------------------------------------
def test_label_zero_only_and_empty_rasters():
    got = check(np.zeros((5, 9), dtype=np.uint32))
    assert got.ringOffsets.tolist() == [0, 0] and got.vertices.shape == (0, 2) and got.rounds == 0 and got.edges == 0
    for shape in ((0, 5), (5, 0)):
        got = check(np.zeros(shape, dtype=np.uint32), maxSegId=2)
        assert got.ringOffsets.tolist() == [0, 0, 0, 0] and got.columns['numParts'].tolist() == [0, 0, 0]


def test_sparse_and_wide_ids():
    got = check(oc.sparse_ids(), maxSegId=oc.SPARSE_MAX)
    assert np.count_nonzero(got.columns['numParts']) == 3 and len(got.ringOffsets) == oc.SPARSE_MAX + 2
    check(oc.wide_ids(), False, maxSegId=oc.WIDE_MAX)


def test_origin_moves_the_vertices_and_nothing_else():
    here = check(oc.scattered_parts())
    moved = check(oc.scattered_parts(), origin=(10, 1000))
    assert np.array_equal(moved.vertices, here.vertices + np.array([10, 1000]))
    for k in ('ringOffsets', 'vertexOffsets', 'ringArea2'):
        assert np.array_equal(getattr(moved, k), getattr(here, k)), k
    far = trace(oc.EXAMPLE, origin=(2 ** 32 - 3, 2 ** 32 - 3))
    assert far.ringArea2.tolist() == oc.EXAMPLE_AREA2 and far.vertices.max() == 2 ** 32


def test_label_above_max_seg_id():
    from pyshepseg_amd import outlines
    seg = np.array(real_raster('seg_final'))
    top = int(seg.max())
    with pytest.raises(outlines.PyShepSegOutlinesError, match='segment id %d is above maxSegId %d' % (top, top - 1)):
        trace(seg, maxSegId=top - 1)
    seg[5:9, 5:9] = top + 7
    seg[127, 127] = 0xFFFFFFF0
    with pytest.raises(outlines.PyShepSegOutlinesError, match='segment id %d is above maxSegId %d' % (0xFFFFFFF0, top)):
        trace(seg, maxSegId=top)
    check(np.array(real_raster('seg_final')), maxSegId=top)


# ---- identities on real label rasters ---------------------------------------------------------------------------------
@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
@pytest.mark.parametrize('name', ['mosaic', 'seg_final', 'random1024'])
def test_identities(name, four):
    from pyshepseg_amd import shapes, shepseg
    seg = real_raster(name)
    got = trace(seg, fourConnected=four)
    s = shapes.calcSegmentShapes(seg)
    assert got.maxSegId == s.maxSegId and got.rounds <= round_bound(got.edges)
    ro = got.ringOffsets
    a2 = np.concatenate([[0], np.cumsum(got.ringArea2)])
    assert np.array_equal(a2[ro[1:]] - a2[ro[:-1]], 2 * s.columns['area'])
    ln = np.concatenate([[0], np.cumsum(oc.ring_lengths(got.vertexOffsets, got.vertices))])
    assert np.array_equal(ln[ro[1:]] - ln[ro[:-1]], s.columns['perimeter'])
    assert got.edges == s.columns['perimeter'].sum()
    assert np.array_equal(oc.rasterise(seg.shape, ro, got.vertexOffsets, got.vertices), seg)
    has = np.flatnonzero(np.diff(ro) > 0)
    assert np.array_equal(has, np.flatnonzero(s.columns['area'])) and np.all(got.ringArea2[ro[has]] > 0)
    nv = np.diff(got.vertexOffsets)
    assert np.all(nv >= 4) and not np.any(nv & 1)
    if name == 'seg_final' and four:
        (clumps, _next) = shepseg.clump(seg, 0, fourConnected=True)
        pairs = np.unique(np.stack([seg.ravel(), clumps.ravel()], axis=1)[seg.ravel() != 0], axis=0)
        parts = np.bincount(pairs[:, 0].astype(np.int64), minlength=got.maxSegId + 1)
        assert s.columns['area'].max() < 10000          # (no segment is cut by the clumping's depth limit)
        assert np.array_equal(got.columns['numParts'], parts)


@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
@pytest.mark.parametrize('name', ['seg_final', 'random256'])
def test_real_rasters_against_the_model(name, four):
    assert_same(trace(real_raster(name), fourConnected=four), real_model(name, four))


# ---- sources ----------------------------------------------------------------------------------------------------------
def test_npy_path_result_object_and_merged_array(tmp_path):
    from pyshepseg_amd import neighbours, tiling
    seg = real_raster('seg_final')
    want = trace(seg)
    path = str(tmp_path / 'labels.npy')
    np.save(path, seg)
    assert_same(trace(path), want)
    res = tiling.TiledSegmentationResult()
    res.segimg = seg
    res.maxSegId = int(seg.max()) + 2               # the result's own maxSegId is taken
    got = trace(res)
    assert got.maxSegId == int(seg.max()) + 2 and np.array_equal(got.ringOffsets[:-2], want.ringOffsets)
    assert np.array_equal(got.vertices, want.vertices)
    S = int(seg.max())
    nb = neighbours.findSegmentNeighbours(seg, True, maxSegId=S)
    m = neighbours.mergeSegments(nb, (np.arange(S + 1) % 3).astype(np.int64), segfile=seg)
    assert m.outDev is None
    assert_same(trace(m, fourConnected=False), oc.reference_outlines(m.segimg, False, m.maxSegId))


def test_device_resident_labels_and_their_merge():
    """labels kept in HBM by the tiled segmentation, read in place; the recoded raster a merge leaves in HBM"""
    from pyshepseg_amd import _lib, tiling, neighbours
    (nrows, ncols) = (300, 902)
    ras = tiling.DeviceRaster.synth(3, 3, nrows, ncols)
    try:
        cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=3)
        rd = tiling.doTiledShepherdSegmentation(ras, tiling._KEEP_ON_DEVICE, tileSize=256, overlapSize=64,
                                                minSegmentSize=30, numClusters=12, fixedKMeansInit=True,
                                                concurrencyCfg=cfg)
        m = None
        try:
            c = _lib.ctx()

            def download(outDev):
                img = np.empty((nrows, ncols), dtype=np.uint32)
                c.check(c._L.shp_dev_download(c.handle, img.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(outDev[0]),
                                              img.nbytes))
                return img
            S = rd.maxSegId
            got = {'own': trace(rd), 'given': trace(rd, maxSegId=S)}
            rd.maxSegId = None                      # the largest label is then found on the device
            got['reduced'] = trace(rd)
            rd.maxSegId = S
            segimg = download(rd.outDev)
            nb = neighbours.findSegmentNeighbours(rd, True, maxSegId=S)
            m = neighbours.mergeSegments(nb, (np.arange(S + 1) % 3).astype(np.int64), segfile=rd)
            assert m.segimg is None and m.outDev is not None
            merged = trace(m)
            mergedimg = download(m.outDev)
            M = m.maxSegId
        finally:
            if m is not None:
                tiling.freeDeviceOutput(m)
            tiling.freeDeviceOutput(rd)
    finally:
        ras.free()
    assert int(segimg.max()) == S
    want = trace(segimg)
    assert np.array_equal(oc.rasterise(segimg.shape, want.ringOffsets, want.vertexOffsets, want.vertices), segimg)
    for key in got:
        assert_same(got[key], want)
    assert_same(merged, trace(mergedimg, maxSegId=M))
    assert np.array_equal(oc.rasterise(mergedimg.shape, merged.ringOffsets, merged.vertexOffsets, merged.vertices), mergedimg)


# ---- entry points -----------------------------------------------------------------------------------------------------
def test_call_order_is_enforced_and_the_other_tables_stay():
    """every refused call fails on the host, before any kernel; outlines leave the context's neighbour table and shape
    table alone"""
    from pyshepseg_amd import _lib, neighbours, shapes
    nb = neighbours.findSegmentNeighbours(nc.EXAMPLE, True)
    serial = neighbours.residentTableSerial()
    assert serial is not None and serial == nb.residentSerial
    c = _lib.ctx()
    L = c._L
    counts = np.full(3, 7, dtype=np.int64)
    out = [np.full(64, 7, dtype=np.int64) for _k in range(4)]

    def refused(rc, what):
        assert rc != 0
        assert what in L.shp_last_error(c.handle).decode()

    def trace_call():
        return L.shp_outline_trace(c.handle, 0, 0, _lib.ptr(counts), None)

    def download_call():
        return L.shp_outline_download(c.handle, *[_lib.ptr(a) for a in out])
    # a shape table begun and accumulated, finished only after the outlines
    c.check(L.shp_shape_begin(c.handle, 3, 0, 0))
    trace(oc.EXAMPLE)                               # traced: a second trace needs new edges, a download does not
    refused(trace_call(), 'shp_outline_edges_dev must come first')
    c.check(download_call())
    assert out[0][:5].tolist() == [0, 0, 1, 2, 3] and out[3][:3].tolist() == oc.EXAMPLE_AREA2
    (edges, bad) = (ctypes.c_int64(0), ctypes.c_uint32(0))
    c.check(L.shp_outline_edges_dev(c.handle, None, 0, 0, 0, 1, ctypes.byref(edges), ctypes.byref(bad)))
    refused(download_call(), 'shp_outline_trace must come first')
    refused(L.shp_outline_trace(c.handle, -1, 0, _lib.ptr(counts), None), 'origin')
    refused(L.shp_outline_trace(c.handle, 0, 0, None, None), 'NULL')
    assert counts.tolist() == [7, 7, 7]
    refused(L.shp_outline_edges_dev(c.handle, None, 0, 0, -1, 1, ctypes.byref(edges), ctypes.byref(bad)), 'max_seg_id')
    refused(L.shp_outline_edges_dev(c.handle, None, 3, 3, 0, 1, ctypes.byref(edges), ctypes.byref(bad)), 'NULL')
    c.check(L.shp_outline_edges_dev(c.handle, None, 0, 0, 0, 1, ctypes.byref(edges), ctypes.byref(bad)))
    c.check(trace_call())
    assert counts.tolist() == [0, 0, 0] and (edges.value, bad.value) == (0, 0)
    c.check(download_call())
    assert out[0][:2].tolist() == [0, 0] and out[1][0] == 0
    # a label above max_seg_id leaves nothing to trace
    (S, sbad) = (ctypes.c_uint32(0), ctypes.c_uint32(0))
    c.check(L.shp_shape_finish(c.handle, ctypes.byref(S), ctypes.byref(sbad), None))
    table = np.full((4, 11), 7, dtype=np.uint64)
    c.check(L.shp_shape_download(c.handle, _lib.ptr(table)))
    assert not table.any()                          # the table begun before the outlines: empty, and still there
    assert neighbours.residentTableSerial() == serial
    red = neighbours.reduceOverNeighbours(nb, [(np.arange(4, dtype=np.float64), [('n', 'count')])])
    assert red['n'].tolist() == [0, 2, 2, 2] and not nb.reduceTimings['uploaded']
    with pytest.raises(Exception, match='above maxSegId'):
        trace(oc.EXAMPLE, maxSegId=2)
    refused(trace_call(), 'shp_outline_edges_dev must come first')
    assert shapes.calcSegmentShapes(oc.EXAMPLE).columns['perimeter'].tolist() == [0, 8, 10, 6]
    check(oc.EXAMPLE)


def test_working_set_is_sized_and_refused_before_it_is_allocated(monkeypatch):
    """shp_outline_need's bytes (5 a pixel; 37 an edge with 16 a vertex and 52 for each of a quarter as many rings at
    their bounds, each buffer with the eighth the context's buffers grow by); a call that does not fit the free memory
    raises with the bytes named before the labels go up, and before the edges' arrays when those do not fit"""
    from pyshepseg_amd import _lib, outlines
    c = _lib.ctx()
    (need, free) = (ctypes.c_int64(0), ctypes.c_int64(0))
    npix = 3 * 2 ** 30
    c.check(c._L.shp_outline_need(c.handle, npix, -1, ctypes.byref(need), ctypes.byref(free)))
    assert 5 * npix <= need.value <= 5 * npix * 9 // 8 + 2 ** 23 and free.value > 2 ** 30
    edges = 2 ** 31
    c.check(c._L.shp_outline_need(c.handle, 0, edges, ctypes.byref(need), ctypes.byref(free)))
    assert (37 + 16 + 13) * edges <= need.value <= (37 + 16 + 13) * edges * 9 // 8 + 2 ** 23
    assert c._L.shp_outline_need(c.handle, 2 ** 32, -1, ctypes.byref(need), ctypes.byref(free)) != 0

    class Library(object):
        """the library, whose buffers would have to grow by a terabyte more from the (after + 1)-th question on"""
        def __init__(self, after):
            (self.after, self.calls) = (after, [])

        def __getattr__(self, name):
            fn = getattr(c._L, name)

            def call(*args):
                self.calls.append(name)
                rc = fn(*args)
                if name == 'shp_outline_need' and self.calls.count(name) > self.after:
                    args[3]._obj.value += 10 ** 12
                return rc
            return call

    class Ctx(object):
        def __init__(self, after):
            (self.handle, self.check, self._L) = (c.handle, c.check, Library(after))

    fake = Ctx(0)
    monkeypatch.setattr(_lib, 'ctx', lambda: fake)
    with pytest.raises(outlines.PyShepSegOutlinesError, match=r'3 x 3 pixels need 1\d{12} bytes of device memory, \d+ are free'):
        outlines.traceSegmentOutlines(oc.EXAMPLE)
    assert fake._L.calls == ['shp_outline_need']
    fake = Ctx(1)
    with pytest.raises(outlines.PyShepSegOutlinesError, match=r'24 edges need 1\d{12} bytes of device memory, \d+ are free'):
        outlines.traceSegmentOutlines(oc.EXAMPLE, maxSegId=3)
    assert 'shp_outline_trace' not in fake._L.calls and fake._L.calls[-2:] == ['shp_outline_need', 'shp_dev_free']
    monkeypatch.undo()
    check(oc.EXAMPLE)


def test_readme_example(tmp_path):
    """the README's lines: outlines into the column dictionary, one id as WKT, chosen ids as GeoJSON"""
    import json
    from pyshepseg_amd import outlines, shapes
    seg = real_raster('mosaic')
    o = outlines.traceSegmentOutlines(seg, fourConnected=True)
    cols = dict(shapes.calcSegmentShapes(seg).columns)
    cols.update(o.columns)
    big = int(np.argsort(cols['area'])[-1])
    wkt = outlines.toWKT(o, big)
    path = str(tmp_path / 'largest.geojson')
    n = outlines.writeGeoJSON(o, path, ids=np.argsort(cols['area'])[-10:], columns=cols)
    assert wkt.startswith('MULTIPOLYGON (((') and n == 10
    with open(path) as f:
        doc = json.load(f)
    assert len(doc['features']) == 10 and doc['features'][-1]['properties']['segId'] == big
    assert doc['features'][-1]['properties']['numParts'] == cols['numParts'][big] >= 1
