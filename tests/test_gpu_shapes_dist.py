"""Shape attributes on row-sharded labels (distributed.deviceShapes, calcSegmentShapesDistributed): rank threads of one
process on one GPU, each with the rows of its cut and the whole raster's histogram, against the one-GPU function on the
whole raster, the numpy definition and the numpy model of the split (shapes_dist_helpers); then the pipeline through
the driver with rank processes.

Not covered here: byte offsets past 2^32 in the table.  They begin at ids above 48.8 M, a 4.3-GB table per rank thread;
'wide-ids' would be 1.5 GB per rank thread for a property (labels past 2^24) the one-GPU test already pins."""
import functools
import os
import types

import numpy as np
import pytest

import dist_cases
import neighbours_dist_helpers as D
import shape_cases as SC
import shapes_dist_helpers as SD
import stats_bands_dist_helpers as H
from pyshepseg_amd import _lib, distributed, shapes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Err = shapes.PyShepSegShapesError


def histOf(seg, S):
    return np.bincount(seg.ravel().astype(np.int64), minlength=S + 1)[:S + 1].astype(np.int64)


@functools.lru_cache(maxsize=None)
def oneGpu(name):
    """the one-GPU shapes of a case's whole raster (computed once; nobody changes them)"""
    (seg, S, _cuts) = SD.caseByName(name)
    return shapes.calcSegmentShapes(seg, maxSegId=S)


def runShapes(seg, cuts, maxSegIds, hists, ranges=None, after=None):
    """deviceShapes in len(cuts) - 1 rank threads (maxSegIds, hists: one per rank); after(rank, comm, c): more work in
    the same thread"""
    (nRows, nCols) = seg.shape
    world = len(cuts) - 1
    ranges = ranges or [(cuts[r], cuts[r + 1]) for r in range(world)]

    def body(rank, comm, c):
        (lo, hi) = ranges[rank]
        d = H.uploadRows(c, seg[lo:hi])
        try:
            info = {}
            s = distributed.deviceShapes(c, comm, d.value, nRows, nCols, (lo, hi), maxSegIds[rank], hists[rank], info=info)
            more = after(rank, comm, c) if after else None
        finally:
            c.check(c._L.shp_dev_free(c.handle, d))
        return s, info, more
    return H.runRankThreads(world, body)


def assertSame(got, whole, ref, what):
    (refC, refS) = ref
    assert list(got.columns) == list(shapes.COUNT_COLUMNS + shapes.DERIVED_COLUMNS) and list(got.sums) == list(shapes.SUM_COLUMNS)
    for k in shapes.COUNT_COLUMNS:
        assert got.columns[k].dtype == np.int64, (what, k)
        assert np.array_equal(got.columns[k], whole.columns[k]) and np.array_equal(got.columns[k], refC[k]), (what, k)
    for k in shapes.SUM_COLUMNS:
        assert got.sums[k].dtype == np.uint64, (what, k)
        assert np.array_equal(got.sums[k], whole.sums[k]) and np.array_equal(got.sums[k], refS[k]), (what, k)
    for k in shapes.DERIVED_COLUMNS:
        assert got.columns[k].dtype == np.float64 and got.columns[k].tobytes() == whole.columns[k].tobytes(), (what, k)


@pytest.mark.parametrize('name', SD.GPU_CASES)
def test_every_rank_gets_the_whole_table(name):
    (seg, S, cuts) = SD.caseByName(name)
    m = SD.model(seg, cuts, S)
    SD.assertReach(name, seg, cuts, S, m)
    whole = oneGpu(name)
    ref = SC.reference_shapes(seg, S)
    world = len(cuts) - 1
    (results, errors) = runShapes(seg, cuts, [S] * world, [histOf(seg, S)] * world)
    assert errors == [None] * world, errors
    for (rank, (s, info, _more)) in enumerate(results):
        assert s.maxSegId == S and s.origin == (0, 0) and s.deviceMs >= 0.0
        assertSame(s, whole, ref, (name, rank))
        assert info == m['info'][rank], (name, rank, info, m['info'][rank])


def test_world_one_is_the_one_gpu_table():
    (seg, S, _cuts) = SD.caseByName('A-w2-four')
    (results, errors) = runShapes(seg, [0, seg.shape[0]], [S], [histOf(seg, S)])
    assert errors == [None], errors
    (s, info, _more) = results[0]
    assertSame(s, oneGpu('A-w2-four'), SC.reference_shapes(seg, S), 'world 1')
    assert (info['exchange_bytes'], info['records_sent'], info['halo_rows']) == (0, 0, 0)
    assert (info['records_picked'], info['straddlers']) == (0, 0)


# ---- errors ---------------------------------------------------------------------------------------------------
def assertAllRaise(results, errors, text):
    assert results == [None] * len(errors)
    for e in errors:
        assert isinstance(e, Err) and str(e) == str(errors[0]) and text in str(e), errors


def test_a_label_above_max_seg_id_on_one_rank_raises_on_every_rank():
    (seg, S) = D.field('A')
    seg = seg.copy()
    cuts = H.cutsOf(3)
    seg[cuts[1] + 20, 7] = S + 20               # both in the middle rank's rows, neither in another rank's halo row
    seg[cuts[1] + 31, 150] = S + 50
    (results, errors) = runShapes(seg, cuts, [S] * 3, [histOf(seg, S)] * 3)
    assertAllRaise(results, errors, 'segment id %d is above maxSegId %d' % (S + 50, S))
    assert str(errors[0]) == 'segment id %d is above maxSegId %d' % (S + 50, S)


def test_overlapping_output_rows_raise_on_every_rank():
    (seg, S) = D.field('A')
    (results, errors) = runShapes(seg, [0, 120, 203], [S] * 2, [histOf(seg, S)] * 2, ranges=[(0, 120), (100, 203)])
    assertAllRaise(results, errors, 'SHEPSEG_SHARD=rows')


def test_a_histogram_below_a_ranks_count_raises_on_every_rank():
    """an id that is whole on one rank, its count lowered by 1: that rank holds more of it than the histogram says"""
    (seg, S, cuts) = SD.caseByName('A-w3-four')
    m = SD.model(seg, cuts, S)
    whole = np.flatnonzero((m['holders'] == 1) & (m['hist'] > 1))
    assert len(whole)
    hist = histOf(seg, S)
    hist[whole[0]] -= 1
    (results, errors) = runShapes(seg, cuts, [S] * 3, [hist] * 3)
    assertAllRaise(results, errors, '1 ids with more pixels on one rank')


def test_a_histogram_above_a_straddlers_area_raises_on_every_rank():
    """a straddler's count raised by 1: every rank sends its part, and the folded area is not the histogram's"""
    (seg, S, cuts) = SD.caseByName('A-w3-four')
    m = SD.model(seg, cuts, S)
    hist = histOf(seg, S)
    hist[np.flatnonzero(m['strad'].any(axis=0))[0]] += 1
    (results, errors) = runShapes(seg, cuts, [S] * 3, [hist] * 3)
    assertAllRaise(results, errors, "1 ids whose area over all ranks is not the histogram's")


def test_different_max_seg_ids_raise_on_every_rank():
    (seg, S, cuts) = SD.caseByName('A-w2-four')
    (results, errors) = runShapes(seg, cuts, [S, S + 1], [histOf(seg, S), histOf(seg, S + 1)])
    assertAllRaise(results, errors, 'different maxSegId')


# ---- the context's other tables ---------------------------------------------------------------------------------
def test_the_share_neighbour_table_and_one_gpu_shapes_stay():
    """a share neighbour table resident in the context survives deviceShapes; a one-GPU calcSegmentShapes in the same
    context before and after gives the same bytes"""
    (seg, S, cuts) = SD.caseByName('A-w2-four')
    small = SC.runs_end_on_lane_63()
    hist = histOf(seg, S)
    col = np.arange(S + 1, dtype=np.float64)

    def body(rank, comm, _c):
        c = _lib.ctx()                          # the context the one-GPU functions of this thread use
        comm.c = c
        (lo, hi) = (cuts[rank], cuts[rank + 1])
        d = H.uploadRows(c, seg[lo:hi])
        try:
            before = shapes.calcSegmentShapes(small)
            share = distributed.deviceNeighbours(c, comm, d.value, seg.shape[0], seg.shape[1], (lo, hi), S)
            s = distributed.deviceShapes(c, comm, d.value, seg.shape[0], seg.shape[1], (lo, hi), S, hist)
            red = distributed.reduceOverNeighboursDistributed(types.SimpleNamespace(c=c), comm, share, [(col, [('n', 'count')])])
            after = shapes.calcSegmentShapes(small)
            return s, before, after, red, share.reduceTimings['uploaded'], share.columns['numNeighbours']
        finally:
            c.check(c._L.shp_dev_free(c.handle, d))
    (results, errors) = H.runRankThreads(2, body)
    assert errors == [None, None], errors
    ref = SC.reference_shapes(seg, S)
    for (rank, (s, before, after, red, uploaded, numNb)) in enumerate(results):
        assertSame(s, oneGpu('A-w2-four'), ref, rank)
        assert uploaded is False and np.array_equal(red['n'], numNb)
        for k in shapes.COUNT_COLUMNS + shapes.DERIVED_COLUMNS:
            assert before.columns[k].tobytes() == after.columns[k].tobytes(), k
        for k in shapes.SUM_COLUMNS:
            assert before.sums[k].tobytes() == after.sums[k].tobytes(), k
        assert np.array_equal(before.columns['area'], SC.reference_shapes(small)[0]['area'])


# ---- through the driver ---------------------------------------------------------------------------------------
def _runDriver(world, transport, tag, tmp_path, env=None):
    dist_cases.runRanks(world, [os.path.join(ROOT, 'tests', 'dist_worker_shapes_gpu.py'), str(tmp_path), transport, tag],
                        tmp_path, 900, extra_env=env)


def _checkDriverRun(world, tmp_path, tag):
    base = str(tmp_path / tag)
    parts = [np.load('%s_rank%d.npz' % (base, r)) for r in range(world)]
    (S, M) = (int(parts[0]['maxSegId']), int(parts[0]['M']))
    mosaic = np.load(base + '_labels.npy')
    assert mosaic.shape == (1500, 1300) and int(mosaic.max()) == S and 0 < M < S
    want = {'s1_': shapes.calcSegmentShapes(base + '_labels.npy', maxSegId=S),
            's2_': shapes.calcSegmentShapes(base + '_merged.npy', maxSegId=M)}
    for (r, q) in enumerate(parts):
        for (pre, w) in want.items():
            for k in shapes.COUNT_COLUMNS:
                assert q[pre + k].dtype == np.int64 and np.array_equal(q[pre + k], w.columns[k]), (tag, r, pre, k)
            for k in shapes.SUM_COLUMNS:
                assert q[pre + k].dtype == np.uint64 and np.array_equal(q[pre + k], w.sums[k]), (tag, r, pre, k)
            for k in shapes.DERIVED_COLUMNS:
                assert q[pre + k].tobytes() == w.columns[k].tobytes(), (tag, r, pre, k)
        assert np.array_equal(q['s1_area'][1:], q['hist'][1:]) and np.array_equal(q['s2_area'][1:], q['newHist'][1:])
        assert np.array_equal(q['s1_perimeter'], q['borderLength'] + q['s1_outerBorder'])
        for pre in ('i1_', 'i2_'):
            assert int(q[pre + 'exchange_bytes']) == int(parts[0][pre + 'exchange_bytes'])
            assert int(q[pre + 'straddlers']) == int(parts[0][pre + 'straddlers'])
    live = sum(1 for q in parts if int(q['outHi']) > int(q['outLo']))
    sent = sum(int(q['i1_records_sent']) for q in parts)
    assert int(parts[0]['i1_exchange_bytes']) == 96 * sent + (8 * 1300 * live if world > 1 else 0)
    print('%s: world %d, %d segments (%d after the merge), %d straddlers in %d records = %d bytes received by every rank '
          '(after the merge: %d straddlers, %d bytes); deviceMs distributed %s, one-GPU %s'
          % (tag, world, S, M, int(parts[0]['i1_straddlers']), sent, int(parts[0]['i1_exchange_bytes']),
             int(parts[0]['i2_straddlers']), int(parts[0]['i2_exchange_bytes']),
             [round(float(q['deviceMs']), 3) for q in parts], [round(float(q['oneGpuMs']), 3) for q in parts]))
    return parts


def test_through_the_driver_two_socket_ranks(tmp_path):
    """segmentation kept on the device -> shapes -> neighbour table -> key merge -> shapes of the merge's objects, two
    socket ranks on GPU 0"""
    _runDriver(2, 'socket', 'rows', tmp_path, env={'SHEPSEG_SHARD': 'rows'})
    parts = _checkDriverRun(2, tmp_path, 'rows')
    assert int(parts[0]['i1_straddlers']) > 0 and sum(int(q['i1_records_sent']) for q in parts) > 0
    assert all(int(q['outHi']) > int(q['outLo']) for q in parts)


def test_through_the_driver_rccl_world_one(tmp_path):
    """the same pipeline with an RcclComm at world size 1 (the communicator on the device)"""
    _runDriver(1, 'rccl', 'rccl', tmp_path)
    parts = _checkDriverRun(1, tmp_path, 'rccl')
    assert int(parts[0]['i1_records_sent']) == 0 and int(parts[0]['i1_exchange_bytes']) == 0
