"""The segment-neighbour table and its reductions on row-sharded labels (distributed.deviceNeighbours,
gatherSegmentNeighbours, reduceOverNeighboursDistributed): rank threads of one process on one GPU, each with the rows
of its cut, against the one-GPU functions on the whole raster, the numpy definition and the numpy model of the split
(neighbours_dist_helpers); then the pipeline through the driver with rank processes."""
import functools
import os
import types

import numpy as np
import pytest

import dist_cases
import neighbour_cases as NC
import neighbour_reduce_cases as RC
import neighbours_dist_helpers as D
import stats_bands_dist_helpers as H
from pyshepseg_amd import _lib, distributed, neighbours

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Err = neighbours.PyShepSegNeighboursError


@functools.lru_cache(maxsize=None)
def oneGpu(name):
    """the one-GPU table of a case's whole raster (computed once; nobody changes it)"""
    (_n, seg, S, _cuts, four) = D.caseByName(name)
    return neighbours.findSegmentNeighbours(seg, fourConnected=four, maxSegId=S)


def runTable(seg, S, cuts, four, after=None):
    """deviceNeighbours in len(cuts) - 1 rank threads; after(rank, comm, c, share): more work in the same thread"""
    (nRows, nCols) = seg.shape

    def body(rank, comm, c):
        (lo, hi) = (cuts[rank], cuts[rank + 1])
        d = H.uploadRows(c, seg[lo:hi])
        try:
            info = {}
            share = distributed.deviceNeighbours(c, comm, d.value, nRows, nCols, (lo, hi), S, fourConnected=four, info=info)
            full = distributed.gatherSegmentNeighbours(comm, share)
            more = after(rank, comm, c, share) if after else None
        finally:
            c.check(c._L.shp_dev_free(c.handle, d))
        return share, full, info, more
    return H.runRankThreads(len(cuts) - 1, body)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', D.CASE_NAMES)
def test_every_rank_gets_the_rows_of_its_share(name):
    (_n, seg, S, cuts, four) = D.caseByName(name)
    m = D.model(seg, cuts, S, four)
    D.assertReach(name, m, S)
    whole = oneGpu(name)
    ref = NC.reference_neighbours(seg, four, S)
    assert same(whole.offsets, ref[0]) and same(whole.neighbours, ref[1]) and same(whole.borderLengths, ref[2])
    cols = whole.columns
    (results, errors) = runTable(seg, S, cuts, four)
    assert errors == [None] * len(errors), errors
    for (rank, (share, full, info, _more)) in enumerate(results):
        want = m['ranks'][rank]
        (lo, hi) = distributed.idRange(rank, len(results), S)
        assert share.idRange == (lo, hi) and share.maxSegId == S and share.fourConnected == four
        # the slice of the one-GPU table, and of the reference (through the model, which assembles to it)
        (a, b) = (int(whole.offsets[lo]), int(whole.offsets[hi]))
        assert same(share.offsets, whole.offsets[lo:hi + 1] - a), (name, rank)
        assert same(share.neighbours, whole.neighbours[a:b]) and same(share.borderLengths, whole.borderLengths[a:b])
        assert same(share.offsets, want['offsets']) and same(share.neighbours, want['neighbours'])
        assert same(share.borderLengths, want['borderLengths'])
        assert same(full.offsets, whole.offsets) and same(full.neighbours, whole.neighbours)
        assert same(full.borderLengths, whole.borderLengths)
        for k in ('numNeighbours', 'borderLength'):
            assert same(share.columns[k], cols[k]), (name, rank, k)
        for k in ('records_local', 'records_home', 'records_sent', 'records_picked', 'entries'):
            assert info[k] == want[k], (name, rank, k, info)
        assert info['halo_rows'] == m['halo_rows'] and info['exchange_bytes'] == m['exchange_bytes'], (name, info)
        if hi > lo:
            (ids, lens) = share.neighboursOf(lo)
            assert same(ids, whole.neighboursOf(lo)[0]) and same(lens, whole.neighboursOf(lo)[1])


def test_world_one_is_the_one_gpu_table():
    (_n, seg, S, _cuts, four) = D.caseByName('A-w2-eight')
    (results, errors) = runTable(seg, S, [0, seg.shape[0]], four)
    assert errors == [None]
    (share, full, info, _more) = results[0]
    whole = oneGpu('A-w2-eight')
    assert same(share.offsets, whole.offsets) and same(share.neighbours, whole.neighbours)
    assert same(share.borderLengths, whole.borderLengths) and same(full.offsets, whole.offsets)
    assert (info['records_sent'], info['records_picked'], info['exchange_bytes'], info['halo_rows']) == (0, 0, 0, 0)
    assert info['records_home'] == info['records_local'] == len(whole.neighbours) // 2


# ---- errors ---------------------------------------------------------------------------------------------------
def test_a_label_above_max_seg_id_on_one_rank_raises_on_every_rank():
    (seg, S) = D.field('A')
    seg = seg.copy()
    cuts = H.cutsOf(3)
    seg[cuts[1] + 20, 7] = S + 20               # both in the middle rank's rows, neither in another rank's halo row
    seg[cuts[1] + 31, 150] = S + 50
    (results, errors) = runTable(seg, S, cuts, True)
    assert results == [None] * 3
    for e in errors:
        assert isinstance(e, Err) and str(e) == 'segment id %d is above maxSegId %d' % (S + 50, S), errors


def test_overlapping_output_rows_raise_on_every_rank():
    (seg, S) = D.field('A')
    ranges = [(0, 120), (100, 203)]

    def body(rank, comm, c):
        (lo, hi) = ranges[rank]
        d = H.uploadRows(c, seg[lo:hi])
        try:
            return distributed.deviceNeighbours(c, comm, d.value, 203, seg.shape[1], (lo, hi), S)
        finally:
            c.check(c._L.shp_dev_free(c.handle, d))
    (results, errors) = H.runRankThreads(2, body)
    assert results == [None] * 2
    for e in errors:
        assert isinstance(e, Err) and 'SHEPSEG_SHARD=rows' in str(e), errors


# ---- the reduction --------------------------------------------------------------------------------------------
def reduceColumns(S):
    """float64 with NaNs, values to ignore and many ties; float32; int64"""
    n = S + 1
    rng = np.random.default_rng(S)
    f64 = RC.real_column(n, 3)
    f64[rng.random(n) < 0.05] = np.nan
    f64[rng.random(n) < 0.05] = -7.0            # the ignoreValue
    tied = rng.random(n) < 0.5
    f64[tied] = np.rint(f64[tied] / 250.0)      # a handful of values: ties for 'nearest', equal minima
    f32 = RC.real_column(n, 4).astype(np.float32)
    f32[rng.random(n) < 0.05] = -7.0
    i64 = RC.integer_column(n, 9, 5, dtype=np.int64)
    return [f64, f32, i64]


def selectionsOf(cols):
    return [(col, [('c%d_%s' % (k, st), st) for st in RC.STATS]) for (k, col) in enumerate(cols)]


def assertSameBits(got, want, what):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), (what, k)


REDUCE_CASES = [('A-w2-four', None), ('A-w3-four', None), ('hot-segment', None), ('hot-segment', [0, 97, 300])]


@functools.lru_cache(maxsize=None)
def oneGpuReduced(name):
    whole = neighbours.findSegmentNeighbours(D.caseByName(name)[1], fourConnected=D.caseByName(name)[4],
                                             maxSegId=D.caseByName(name)[2])
    return neighbours.reduceOverNeighbours(whole, selectionsOf(reduceColumns(whole.maxSegId)), ignoreValue=-7.0,
                                           missingStatsValue=-1234.5)


@pytest.mark.parametrize('name,cuts', REDUCE_CASES)
def test_reduction_is_bit_equal_on_every_rank(name, cuts):
    (_n, seg, S, caseCuts, four) = D.caseByName(name)
    cuts = cuts or caseCuts
    want = oneGpuReduced(name)
    if name == 'hot-segment':
        whole = oneGpu(name)
        assert int(np.diff(whole.offsets).max()) == 22500 > RC.CHUNK > RC.LONG and -(-22500 // RC.CHUNK) == 6
        assert all(r['records_local'] > 0 for r in D.model(seg, cuts, S, four)['ranks'])
    sel = selectionsOf(reduceColumns(S))

    def after(rank, comm, c, share):
        out = distributed.reduceOverNeighboursDistributed(types.SimpleNamespace(c=c), comm, share, sel, ignoreValue=-7.0,
                                                          missingStatsValue=-1234.5)
        return out, dict(share.reduceTimings)
    (results, errors) = runTable(seg, S, cuts, four, after)
    assert errors == [None] * len(errors), errors
    for (rank, (_share, _full, _info, (out, timings))) in enumerate(results):
        assertSameBits(out, want, (name, rank))
        assert timings['uploaded'] is False


def test_share_table_and_one_gpu_table_do_not_pass_for_each_other():
    """one context per rank holds a share table, then a one-GPU table of another raster, then another share table"""
    (_n, seg, S, cuts, four) = D.caseByName('A-w2-four')
    want = oneGpuReduced('A-w2-four')
    sel = selectionsOf(reduceColumns(S))
    small = NC.enclosed_by_zeros()
    smallCol = np.array([5.0, 1.0, 4.0, 9.0])
    smallSel = [(smallCol, [('m', 'mean'), ('n', 'nearest'), ('b', 'border')])]
    smallTable = neighbours.findSegmentNeighbours(small, maxSegId=3)
    smallWant = neighbours.reduceOverNeighbours(smallTable, smallSel)
    assert smallWant['m'].tolist() == [-9999.0, 4.0, 1.0, -9999.0] and smallWant['b'].tolist() == [0, 10, 10, 0]

    def body(rank, comm, _c):
        c = _lib.ctx()                          # the context the one-GPU functions of this thread use
        comm.c = c
        eng = types.SimpleNamespace(c=c)
        (lo, hi) = (cuts[rank], cuts[rank + 1])
        d = H.uploadRows(c, seg[lo:hi])
        d2 = H.uploadRows(c, small[20 * rank:20 * rank + 20])
        try:
            share = distributed.deviceNeighbours(c, comm, d.value, seg.shape[0], seg.shape[1], (lo, hi), S, fourConnected=four)
            assert neighbours.residentTableSerial() is None         # a share table is no finished one-GPU table
            steps = []
            first = distributed.reduceOverNeighboursDistributed(eng, comm, share, sel, ignoreValue=-7.0, missingStatsValue=-1234.5)
            steps.append(share.reduceTimings['uploaded'])
            # a one-GPU table in the same context: it reduces over its own rows, and the share table stays
            nb = neighbours.findSegmentNeighbours(small, maxSegId=3)
            assert nb.residentSerial is not None and nb.residentSerial != share.residentSerial
            got = neighbours.reduceOverNeighbours(nb, smallSel)
            steps.append(nb.reduceTimings['uploaded'])
            second = distributed.reduceOverNeighboursDistributed(eng, comm, share, sel, ignoreValue=-7.0, missingStatsValue=-1234.5)
            steps.append(share.reduceTimings['uploaded'])
            # another share table in the context: the first is uploaded again, the one-GPU table as well
            other = distributed.deviceNeighbours(c, comm, d2.value, 40, small.shape[1], (20 * rank, 20 * rank + 20), 3)
            third = distributed.reduceOverNeighboursDistributed(eng, comm, share, sel, ignoreValue=-7.0, missingStatsValue=-1234.5)
            steps.append(share.reduceTimings['uploaded'])
            got2 = neighbours.reduceOverNeighbours(nb, smallSel)
            steps.append(nb.reduceTimings['uploaded'])
            otherOut = distributed.reduceOverNeighboursDistributed(eng, comm, other, smallSel)
            steps.append(other.reduceTimings['uploaded'])
            return first, second, third, got, got2, otherOut, steps
        finally:
            for p in (d, d2):
                c.check(c._L.shp_dev_free(c.handle, p))
    (results, errors) = H.runRankThreads(2, body)
    assert errors == [None, None], errors
    for (rank, (first, second, third, got, got2, otherOut, steps)) in enumerate(results):
        for out in (first, second, third):
            assertSameBits(out, want, rank)
        for out in (got, got2, otherOut):
            assertSameBits(out, smallWant, rank)
        assert steps == [False, False, False, True, True, True], steps


# ---- through the driver ---------------------------------------------------------------------------------------
def _runDriver(world, transport, tag, tmp_path, env=None):
    dist_cases.runRanks(world, [os.path.join(ROOT, 'tests', 'dist_worker_neighbours_gpu.py'), str(tmp_path), transport, tag],
                        tmp_path, 900, extra_env=env)


def _checkDriverRun(world, tmp_path, tag):
    base = str(tmp_path / tag)
    parts = [np.load('%s_rank%d.npz' % (base, r)) for r in range(world)]
    mosaic = np.load(base + '_labels.npy')
    S = int(parts[0]['maxSegId'])
    assert mosaic.shape == (1500, 1300) and int(mosaic.max()) == S
    whole = neighbours.findSegmentNeighbours(mosaic, maxSegId=S)
    at = 0
    (ids, lens, offs) = ([], [], [np.zeros(1, dtype=np.int64)])
    for (r, q) in enumerate(parts):
        assert (int(q['idLo']), int(q['idHi'])) == distributed.idRange(r, world, S)
        offs.append(q['offsets'][1:] + at)
        at += int(q['offsets'][-1])
        ids.append(q['neighbours'])
        lens.append(q['borderLengths'])
    assert same(np.concatenate(offs), whole.offsets) and same(np.concatenate(ids), whole.neighbours)
    assert same(np.concatenate(lens), whole.borderLengths)
    mean = parts[0]['mean1']
    assert mean.dtype == np.float32 and mean.shape == (S + 1,)
    want = neighbours.reduceOverNeighbours(whole, [(mean, [('bm', 'bordermean'), ('near', 'nearest')])])
    cols = whole.columns
    for (r, q) in enumerate(parts):
        assert same(q['mean1'], mean)
        for k in ('bm', 'near'):
            assert q[k].dtype == want[k].dtype and np.array_equal(q[k].view(np.uint64), want[k].view(np.uint64)), (tag, r, k)
        for k in ('numNeighbours', 'borderLength'):
            assert same(q[k], cols[k]), (tag, r, k)
    sent = sum(int(q['records_sent']) for q in parts)
    live = sum(1 for q in parts if int(q['outHi']) > int(q['outLo']))
    for q in parts:
        assert int(q['exchange_bytes']) == 16 * sent + (4 * 1300 * live if world > 1 else 0)
    print('%s: world %d, %d segments, %d entries, %d travelling distinct pairs = %d bytes received by every rank; '
          'deviceMs distributed %s, one-GPU %s' % (tag, world, S, len(whole.neighbours), sent, 16 * sent,
                                                   [round(float(q['deviceMs']), 3) for q in parts],
                                                   [round(float(q['oneGpuMs']), 3) for q in parts]))
    return parts


def test_through_the_driver_two_socket_ranks(tmp_path):
    """segmentation kept on the device -> neighbour table -> mean column -> reduction, two socket ranks on GPU 0"""
    _runDriver(2, 'socket', 'rows', tmp_path, env={'SHEPSEG_SHARD': 'rows'})
    parts = _checkDriverRun(2, tmp_path, 'rows')
    assert sum(int(q['records_sent']) for q in parts) > 0 and all(int(q['outHi']) > int(q['outLo']) for q in parts)


def test_through_the_driver_rccl_world_one(tmp_path):
    """the same pipeline with an RcclComm at world size 1 (the communicator on the device)"""
    _runDriver(1, 'rccl', 'rccl', tmp_path)
    parts = _checkDriverRun(1, tmp_path, 'rccl')
    assert int(parts[0]['records_sent']) == 0
