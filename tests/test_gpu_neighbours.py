"""GPU: neighbours.findSegmentNeighbours against the numpy definition (tests/neighbour_cases.py), array for array with
numpy.array_equal: everything is integer, nothing has a tolerance.  The kernel counts the pairs of 32 x 64 patches
in an LDS hash table, so the shapes below are chosen by where that can go wrong: pairs across patch edges and
corners, patches whose pairs do not fit the table, one pair or one segment that is everywhere, ids far apart.

Paths taken only past a threshold have a case that crosses it on purpose: a patch with exactly 1023, 1024 (table full)
and 1025 (first overflow) distinct pairs, and one whose 1024 pairs share a home slot (the last probe of the trip round
the table); a row block that does not fit the record buffer of a fresh context, with and without earlier records to
keep; one pair in hundreds of sorted records (the reduction across wavefronts and workgroups); a segment with 22 500
smaller neighbours; labels past 2^24 (four sort passes); row blocks that end on a patch row; the call orders the C
entry points refuse.  Which route every patch took, and that a block run twice
neither lost nor doubled records, shows in ``recordsSorted``: it must EQUAL the count of the numpy model
neighbour_cases.patch_records.

Border lengths of 2^32 and more (from a raster the 64-bit sums need over 10^9 pixel pairs of one pair) are reached
through the contraction of hand-built tables: tests/test_gpu_merge_tables.py and tests/test_gpu_merge_tables_dist.py
put non-zero high words through k_nbr_reduce (its 64-bit instantiation, which the share tables use) and the share merge.  Not covered: labels of
2^31 and more in a successful table (its offsets alone are 16 GB)."""
import ctypes
import functools
import os
import threading

import numpy as np
import pytest

import neighbour_cases as nc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize('four', [True, False], ids=['4conn', '8conn'])


def find(seg, four=True, **kw):
    from pyshepseg_amd import neighbours
    return neighbours.findSegmentNeighbours(seg, fourConnected=four, **kw)


def block_rows(seg, chunkPixels=None):
    """the rows findSegmentNeighbours puts in a block (None: the default block holds all of these rasters)"""
    return None if chunkPixels is None else max(1, chunkPixels // max(seg.shape[1], 1))


def assert_table(got, want, four=None, records=None):
    """records: the model's record count, which recordsSorted must equal"""
    (offsets, nbrs, lens) = want
    assert got.offsets.dtype == np.int64 and got.neighbours.dtype == np.uint32 and got.borderLengths.dtype == np.int64
    assert got.maxSegId == len(offsets) - 2
    assert np.array_equal(got.offsets, offsets)
    assert np.array_equal(got.neighbours, nbrs)
    assert np.array_equal(got.borderLengths, lens)
    assert 2 * got.pairsSeen == int(lens.sum())
    assert len(nbrs) // 2 <= got.recordsSorted <= got.pairsSeen
    if records is not None:
        assert got.recordsSorted == records
    if four is not None:
        assert got.fourConnected is four


def check(seg, four, maxSegId=None, chunkPixels=None):
    got = find(seg, four, maxSegId=maxSegId, chunkPixels=chunkPixels)
    assert_table(got, nc.reference_neighbours(seg, four, maxSegId), four,
                 records=nc.patch_records(seg, four, block_rows(seg, chunkPixels))[1])
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


@functools.lru_cache(maxsize=None)
def real_records(name, four, rows=None):
    return nc.patch_records(real_raster(name), four, rows)[1]


def in_fresh_context(fn):
    """fn() in a new thread: _lib.ctx() is per thread, so its record buffer has never grown.  The thread's context is
    closed before the thread ends."""
    from pyshepseg_amd import _lib
    out = {}

    def run():
        try:
            try:
                out['value'] = fn()
            finally:
                _lib.ctx().close()
        except BaseException as e:          # (an AssertionError of fn belongs to the test)
            out['error'] = e
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if 'error' in out:
        raise out['error']
    return out['value']


# ---- 1: the worked example ----------------------------------------------------------------------------------
@BOTH
def test_example(four):
    got = find(nc.EXAMPLE, four)
    assert got.offsets.tolist() == nc.EXAMPLE_OFFSETS
    assert got.neighbours.tolist() == nc.EXAMPLE_NEIGHBOURS
    assert got.borderLengths.tolist() == nc.EXAMPLE_LENGTHS[four]
    assert got.maxSegId == 3 and got.fourConnected is four
    assert got.recordsSorted == nc.patch_records(nc.EXAMPLE, four)[1] == 3 and got.blocksRerun == 0
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
    assert_table(find(real_raster(name), four), real_reference(name, four), four, records=real_records(name, four))


def test_random_1024():
    got = find(real_raster('random1024'), False)
    assert len(got.neighbours) == 8352378
    assert_table(got, real_reference('random1024', False), False, records=real_records('random1024', False))


# ---- 10: the table does not depend on the row blocks ---------------------------------------------------------
@pytest.mark.parametrize('rows', [1, 7, 32, 33, 64])
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
    assert len(want[1]) // 2 <= got.recordsSorted <= got.pairsSeen
    assert got.recordsSorted == real_records(name, four, rows)


@BOTH
def test_npy_path_and_result_object(four, tmp_path):
    from pyshepseg_amd import tiling
    seg = real_raster('mosaic')
    path = str(tmp_path / 'labels.npy')
    np.save(path, seg)
    want = real_reference('mosaic', four)
    assert_table(find(path, four), want, four, records=real_records('mosaic', four))
    assert_table(find(path, four, chunkPixels=33 * seg.shape[1]), want, four, records=real_records('mosaic', four, 33))
    res = tiling.TiledSegmentationResult()
    res.segimg = seg
    assert_table(find(res, four, chunkPixels=7 * seg.shape[1]), want, four, records=real_records('mosaic', four, 7))


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
            assert_table(got[(four, rows)], want, four, records=nc.patch_records(segimg, four, rows)[1])
        assert_table(find(segimg, four), want, four, records=nc.patch_records(segimg, four)[1])


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
    assert_table(find(solid, four, maxSegId=9), nc.reference_neighbours(solid, four, 9), four, records=0)


# ---- 12: the hash table at its boundary -----------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize('n', [1023, 1024, 1025])
def test_table_fill(n, four):
    """one patch with exactly n distinct pairs and more runs than that: 1024 fills every slot, 1025 is the first to
    overflow, and the patch then hands over its runs.  (How far the last pair of 1024 has to probe depends on these
    labels' home slots and on the order of arrival: at most 1012 slots with 4-connectivity.  test_table_wrap is
    the case that needs the whole trip round the table.)"""
    seg = nc.table_fill(n, four)
    (per, total) = nc.patch_records(seg, four)
    (D, R) = per[4, :2].tolist()
    assert D == n and R != D and not np.delete(per, 4, axis=0).any()
    got = check(seg, four)
    assert got.recordsSorted == total == (n if n <= 1024 else R)


@BOTH
def test_table_wrap(four):
    """1024 distinct pairs that all have the same home slot (the hash of csrc/neighbours.h, in numpy as
    neighbour_cases.pair_home): they fill 1024 slots in a row, so whichever of them arrives last is placed only by
    the 1024th probe.  A probe loop that gives up one slot early sends the patch down the overflow route, and its 1025
    runs show in recordsSorted."""
    seg = nc.table_wrap()
    (per, total) = nc.patch_records(seg, four)
    assert per[4].tolist()[:2] == [1024, 1025] and total == (1024 if four else 1025)
    got = check(seg, four)
    assert got.recordsSorted == total


# ---- 13: one pair in many sorted records ----------------------------------------------------------------------
@BOTH
def test_zone_stripes(four):
    """nine pairs, each with 203 or more records in 1-row blocks: the runs of the sorted records start at lane
    offsets that move (203 mod 64 = 11) and cross wavefronts and workgroups"""
    seg = nc.zone_stripes()
    got = check(seg, four, chunkPixels=seg.shape[1])
    assert got.recordsSorted == (1827 if four else 2635)
    assert len(got.neighbours) == 18 and int(got.borderLengths.max()) == (12789 if four else 38241)
    whole = check(seg, four)
    assert whole.recordsSorted == (63 if four else 91)
    assert np.array_equal(whole.borderLengths, got.borderLengths)


@BOTH
def test_stripes_in_one_row_blocks(four):
    """1285 records of one pair"""
    seg = nc.stripes()
    got = check(seg, four, chunkPixels=seg.shape[1])
    assert got.recordsSorted == 1285 and got.neighbours.tolist() == [2, 1]


# ---- 14: a long run of smaller neighbours ---------------------------------------------------------------------
@BOTH
def test_hot_segment_with_the_largest_id(four):
    got = check(nc.hot_segment_top(), four)
    (ids, lens) = got.neighboursOf(22502)
    assert len(ids) == 22500 and ids.tolist() == list(range(2, 22502))
    assert got.recordsSorted == (22500 if four else 23100)


# ---- 15: a row block that does not fit the record buffer ---------------------------------------------------------
@BOTH
def test_block_rerun_keeps_earlier_records(four):
    """a fresh context guesses 32 * 128 / 8 + 1024 = 1536 records for the first 32-row block; the first two blocks
    fit, the third needs over four times the room: the buffer is regrown with the records of two blocks kept, the
    counters are put back and the block runs again"""
    seg = nc.calm_then_busy()
    want = nc.reference_neighbours(seg, four)
    records = nc.patch_records(seg, four, 32)[1]
    assert records == (8392 if four else 16514)

    def blocks():
        got = find(seg, four, chunkPixels=32 * 128)
        again = find(seg, four, chunkPixels=32 * 128)
        return (got, again)
    (got, again) = in_fresh_context(blocks)
    assert_table(got, want, four, records=records)
    assert got.pairsSeen == int(want[2].sum()) // 2
    # (this figure, and the ones below, follow from run_nbr_accumulate's first guess and buf_ensure's slack, worked
    #  out in LABNOTES 2026-10-17, fourth entry: a change of that policy moves them with no kernel at fault)
    assert got.blocksRerun == 1
    # a buffer reused from an earlier table: nothing runs twice, the table is the same
    assert again.blocksRerun == 0
    assert_table(again, want, four, records=records)


@BOTH
def test_block_rerun_with_nothing_to_keep(four):
    seg = nc.calm_then_busy()
    want = nc.reference_neighbours(seg, four)
    got = in_fresh_context(lambda: find(seg, four))
    assert_table(got, want, four, records=nc.patch_records(seg, four)[1])
    assert got.blocksRerun == 1           # (run_nbr_accumulate's first guess: 96 * 128 / 8 + 1024 < 8392)
    # upside down in 32-row blocks: the first block runs twice, the later ones fit what it left
    flipped = np.ascontiguousarray(seg[::-1])
    got = in_fresh_context(lambda: find(flipped, four, chunkPixels=32 * 128))
    assert_table(got, nc.reference_neighbours(flipped, four), four, records=nc.patch_records(flipped, four, 32)[1])
    # (the second block's guess, the first block's count + 1/8, regrows BEFORE that block runs: no rerun of it)
    assert got.blocksRerun == 1


# ---- 16: four sort passes ----------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize('maxSegId', [None, nc.WIDE_MAX])
def test_ids_past_2_to_24(maxSegId, four):
    got = check(nc.wide_ids(), four, maxSegId=maxSegId)
    assert got.maxSegId == ((1 << 24) + 9 if maxSegId is None else nc.WIDE_MAX)
    assert len(got.neighbours) == 6


# ---- 17: the order of the calls ----------------------------------------------------------------------------------
def test_call_order_is_enforced():
    """every refused call fails on the host, before any kernel"""
    from pyshepseg_amd import _lib

    def calls():
        c = _lib.ctx()
        L = c._L
        (S, nent, bad) = (ctypes.c_uint32(0), ctypes.c_int64(0), ctypes.c_uint32(0))
        counters = np.zeros(3, dtype=np.int64)
        offsets = np.full(2, -1, dtype=np.int64)

        def finish():
            return L.shp_nbr_finish(c.handle, ctypes.byref(S), ctypes.byref(nent), ctypes.byref(bad),
                                    _lib.ptr(counters), None)

        def refused(rc, what):
            assert rc != 0
            assert what in L.shp_last_error(c.handle).decode()
        refused(L.shp_nbr_accumulate_dev(c.handle, None, 1, 1, 0), 'shp_nbr_begin must come first')
        refused(finish(), 'shp_nbr_begin must come first')
        refused(L.shp_nbr_download(c.handle, _lib.ptr(offsets), None, None), 'shp_nbr_finish must come first')
        c.check(L.shp_nbr_begin(c.handle, -1, 1))
        refused(L.shp_nbr_download(c.handle, _lib.ptr(offsets), None, None), 'shp_nbr_finish must come first')
        assert offsets.tolist() == [-1, -1]
        c.check(finish())
        assert (S.value, nent.value, bad.value, counters.tolist()) == (0, 0, 0, [0, 0, 0])
        refused(L.shp_nbr_accumulate_dev(c.handle, None, 1, 1, 0), 'shp_nbr_begin must come first')
        refused(finish(), 'shp_nbr_begin must come first')
        c.check(L.shp_nbr_download(c.handle, _lib.ptr(offsets), None, None))
        assert offsets.tolist() == [0, 0]
        return [find(nc.EXAMPLE, four) for four in (True, False)]
    for (four, got) in zip((True, False), in_fresh_context(calls)):
        assert_table(got, nc.reference_neighbours(nc.EXAMPLE, four), four, records=nc.patch_records(nc.EXAMPLE, four)[1])
        assert got.neighbours.tolist() == nc.EXAMPLE_NEIGHBOURS and got.blocksRerun == 0
