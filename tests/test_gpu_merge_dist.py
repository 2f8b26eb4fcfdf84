"""Segments merged on the id-sharded neighbour table (distributed.deviceMerge, mergeRule, aggregateToGroupsDistributed):
rank threads of one process on one GPU, each with the rows of its cut and the share deviceNeighbours gave it, against
the one-GPU functions on the whole raster and the numpy model of the split (merge_dist_cases); then the pipeline
through the driver with rank processes."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest

import aggregate_cases as AC
import dist_cases
import merge_cases as mc
import merge_dist_cases as MD
import neighbour_cases as NC
import neighbours_dist_helpers as D
import similar_cases as sc
import stats_bands_dist_helpers as H
from pyshepseg_amd import _lib, distributed, neighbours

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Err = neighbours.PyShepSegNeighboursError


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def cutsFor(nRows, world):
    return [int(round(nRows * r / world)) for r in range(world + 1)]


def fetchRows(c, res):
    """the recoded rows of a rank's result, its device buffer released"""
    if res.outDev is None:
        return np.zeros((0, 0), dtype=np.uint32)
    (p, h, w, nbytes) = res.outDev
    out = np.empty((h, w), dtype=np.uint32)
    c.check(c._L.shp_dev_download(c.handle, _lib.ptr(out), ctypes.c_void_p(p), out.nbytes))
    c.check(c._L.shp_dev_free(c.handle, ctypes.c_void_p(p)))
    res.outDev = None
    return out


def runMerge(seg, S, cuts, four, ruleArgs, withRows=True, after=None, mergeSeg=None, mergeRanges=None):
    """deviceNeighbours, then deviceMerge under mergeRule(share, **ruleArgs) in len(cuts) - 1 rank threads;
    after(rank, comm, c, share, res): more work in the same thread.  mergeSeg / mergeRanges: another raster / other
    row ranges for the recode."""
    (nRows, nCols) = seg.shape
    world = len(cuts) - 1

    def body(rank, comm, c):
        (lo, hi) = (cuts[rank], cuts[rank + 1])
        d = H.uploadRows(c, seg[lo:hi])
        d2 = None
        try:
            share = distributed.deviceNeighbours(c, comm, d.value, nRows, nCols, (lo, hi), S, fourConnected=four)
            rule = distributed.mergeRule(share, **ruleArgs)
            info = {}
            (rows, dRows) = ((lo, hi), d)
            if mergeRanges is not None:
                rows = mergeRanges[rank]
            if mergeSeg is not None or mergeRanges is not None:
                d2 = H.uploadRows(c, (seg if mergeSeg is None else mergeSeg)[rows[0]:rows[1]])
                dRows = d2
            if withRows:
                res = distributed.deviceMerge(c, comm, share, rule, dRows.value if rows[1] > rows[0] else 0, nRows, nCols,
                                              rows, info=info)
            else:
                res = distributed.deviceMerge(c, comm, share, rule, info=info)
            recoded = fetchRows(c, res)
            more = after(rank, comm, c, share, res) if after else None
        finally:
            for p in (d, d2):
                if p is not None:
                    c.check(c._L.shp_dev_free(c.handle, p))
        return res, recoded, info, more
    return H.runRankThreads(world, body)


@functools.lru_cache(maxsize=None)
def wholeTable(name, four):
    case = [c for c in mc.CASES if c.name == name][0]
    (seg, S, keys, size, table) = mc.build(case, four)
    return (case, seg, S, keys, size, table)


def assertGroups(res, want, what, hist=True):
    assert res.maxSegId == want.maxSegId and res.links == want.links and res.recordsSorted == want.recordsSorted, what
    for k in ('recode', 'representative', 'groupSize'):
        assert same(getattr(res, k), getattr(want, k)), (what, k)
    if hist:
        assert (res.hist is None) == (want.hist is None), what
        if want.hist is not None:
            assert same(res.hist, want.hist), what


def assertShare(res, whole, rank, world, what):
    """the rank's share of the contracted table is the rows of the one-GPU result's table ``whole``"""
    M = whole.maxSegId
    (lo, hi) = distributed.idRange(rank, world, M)
    nshare = res.neighbours
    assert nshare.idRange == (lo, hi) and nshare.maxSegId == M, what
    (a, b) = (int(whole.offsets[lo]), int(whole.offsets[hi]))
    assert same(nshare.offsets, whole.offsets[lo:hi + 1] - a), what
    assert same(nshare.neighbours, whole.neighbours[a:b]) and same(nshare.borderLengths, whole.borderLengths[a:b]), what
    cols = whole.columns
    for k in ('numNeighbours', 'borderLength'):
        assert same(nshare.columns[k], cols[k]), (what, k)


def checkAgainstOneGpuAndModel(seg, S, four, cuts, ruleArgs, oneGpu, link, size, mutual=False, what=None):
    """every rank of a run against the one-GPU result ``oneGpu`` (with .segimg) and the model of the split"""
    table = NC.reference_neighbours(seg, four, S)
    world = len(cuts) - 1
    m = MD.model(table, link(table), world, size, mutual=mutual)
    (results, errors) = runMerge(seg, S, cuts, four, ruleArgs)
    assert errors == [None] * world, errors
    for (rank, (res, recoded, info, _more)) in enumerate(results):
        assertGroups(res, oneGpu, (what, rank))
        assertGroups(res, m['groups'], (what, rank, 'model'), hist=size is not None)
        assertShare(res, oneGpu.neighbours, rank, world, (what, rank))
        want = m['ranks'][rank]
        assert same(res.neighbours.offsets, want['offsets']) and same(res.neighbours.neighbours, want['neighbours'])
        assert same(res.neighbours.borderLengths, want['borderLengths'])
        (lo, hi) = (cuts[rank], cuts[rank + 1])
        assert res.rowRange == (lo, hi)
        if hi > lo:
            assert same(recoded, oneGpu.recode[seg[lo:hi]]) and same(recoded, oneGpu.segimg[lo:hi]), (what, rank)
        else:
            assert res.outDev is None and recoded.size == 0
        if size is None:
            assert same(res.hist, np.bincount(oneGpu.recode[seg].ravel(), minlength=res.maxSegId + 1).astype(np.int64))
        deviceMs = info.pop('deviceMs')
        assert info == MD.info_of(m, rank), (what, rank, info, MD.info_of(m, rank))
        assert set(deviceMs) >= {'hook', 'pairs', 'pairhook', 'renumber', 'contract', 'recode'}
    return (results, m)


# ---- the key rule ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oneGpuKeyMerge(name, four, keyKind):
    (case, seg, S, keys, size, _table) = wholeTable(name, four)
    if keyKind == 'mod2':
        keys = np.arange(S + 1) % 2
    nb = neighbours.findSegmentNeighbours(seg, fourConnected=four, maxSegId=S)
    return neighbours.mergeSegments(nb, keys, ignoreKey=case.ignoreKey, minBorder=case.minBorder, segSize=size, segfile=seg)


def keyCase(name, four, world, keyKind=None, cuts=None):
    (case, seg, S, keys, size, _table) = wholeTable(name, four)
    if keyKind == 'mod2':
        keys = np.arange(S + 1) % 2
    ruleArgs = dict(keyColumn=keys, ignoreKey=case.ignoreKey, minBorder=case.minBorder, segSize=size)

    def link(table):
        return MD.key_links(table, keys, case.ignoreKey, case.minBorder, size)
    cuts = cuts or cutsFor(seg.shape[0], world)
    return checkAgainstOneGpuAndModel(seg, S, four, cuts, ruleArgs, oneGpuKeyMerge(name, four, keyKind), link, size,
                                      what=(name, four, world, keyKind))


REACH = [('column_permuted', True, None), ('column_permuted', True, 'mod2'), ('through_a_third', True, None),
         ('through_a_third', False, None), ('star_alternating', True, None), ('star_alternating', False, None)]


@pytest.mark.parametrize('world', [1, 2, 3])
@pytest.mark.parametrize('name,four,keyKind', REACH)
def test_key_merge_on_the_cases_that_need_the_exchange(name, four, keyKind, world):
    (results, m) = keyCase(name, four, world, keyKind)
    pairs = [r['forest_pairs'] for r in m['ranks']]
    if name == 'column_permuted' and four and world > 1:
        assert pairs == {(None, 2): [3089, 1007], (None, 3): [2288, 1367, 441], ('mod2', 2): [1569, 515],
                         ('mod2', 3): [1187, 665, 232]}[(keyKind, world)]
    if name == 'through_a_third' and four and world == 3:
        assert pairs == [0, 1, 1]
    if world == 1:
        (res, _rows, info, _more) = results[0]
        assert info['records_sent'] == 0 and info['forest_pairs'] == pairs[0] > 0


@pytest.mark.parametrize('name,world,cuts', [
    ('row_descending', 2, [0, 1, 1]), ('no_segments', 3, None), ('one_segment', 3, None), ('drawn_large_ignore', 2, None),
    ('drawn_large_ignore', 3, None), ('half_planes_300', 2, None), ('half_planes_301', 2, None)])
def test_key_merge_on_the_small_and_the_drawn_cases(name, world, cuts):
    (results, m) = keyCase(name, True, world, cuts=cuts)
    M = m['groups'].maxSegId
    if name in ('no_segments', 'one_segment'):
        assert M == {'no_segments': 0, 'one_segment': 1}[name]
        assert [r['entries'] for r in m['ranks']] == [0] * world
    if name.startswith('half_planes'):
        assert M == {'half_planes_300': 1, 'half_planes_301': 2}[name]


@functools.lru_cache(maxsize=None)
def fieldA():
    (seg, S) = D.field('A')
    size = np.bincount(seg.ravel(), minlength=S + 1).astype(np.int64)
    assert int((size[1:] == 0).sum()) >= 3          # (ids held by nobody)
    return (seg, S, size)


@functools.lru_cache(maxsize=None)
def oneGpuFieldA():
    (seg, S, size) = fieldA()
    nb = neighbours.findSegmentNeighbours(seg, maxSegId=S)
    return neighbours.mergeSegments(nb, np.arange(S + 1) % 3, segSize=size, segfile=seg)


@pytest.mark.parametrize('cuts', [H.cutsOf(2), H.cutsOf(3), [0, 100, 100, 203]])
def test_key_merge_on_the_field_with_sizes(cuts):
    (seg, S, size) = fieldA()
    keys = np.arange(S + 1) % 3
    checkAgainstOneGpuAndModel(seg, S, True, cuts, dict(keyColumn=keys, segSize=size), oneGpuFieldA(),
                               lambda table: MD.key_links(table, keys, segSize=size), size, what=('A', cuts))


def test_world_one_is_merge_segments_array_for_array():
    (seg, S, size) = fieldA()
    want = oneGpuFieldA()
    (results, errors) = runMerge(seg, S, [0, seg.shape[0]], True, dict(keyColumn=np.arange(S + 1) % 3, segSize=size))
    assert errors == [None], errors
    (res, recoded, info, _more) = results[0]
    assertGroups(res, want, 'world 1')
    for k in ('offsets', 'neighbours', 'borderLengths'):
        assert same(getattr(res.neighbours, k), getattr(want.neighbours, k)), k
    assert same(recoded, want.segimg)
    assert info['records_sent'] == 0 == info['records_picked'] and info['exchange_bytes'] == 8 * info['forest_pairs'] > 0
    assert info['records_home'] == info['records_local'] == len(want.neighbours.neighbours) // 2
    assert info['records_entries'] == want.recordsSorted and info['links'] == want.links


# ---- the similarity rule --------------------------------------------------------------------------------------
def similarInputs(kind):
    """(seg, S, segSize or None, columns, star hub or None) of the rasters the similarity rule runs on"""
    if kind == 'drawn_large':
        seg = NC.random_labels((257, 300), 3000, 12)
        S = int(seg.max())
        return (seg, S, None, sc.integer_columns(S, 2, 5, top=3), None)
    if kind == 'A':
        (seg, S, size) = fieldA()
        cols = sc.integer_columns(S, 2, 6, top=4)
        cols[0][::17] = np.nan
        cols[1][5::23] = -7.0
        return (seg, S, size, cols, None)
    seg = NC.hot_segment()
    S = int(seg.max())
    hub = int(np.argmax(np.bincount(seg.ravel(), minlength=S + 1)))
    return (seg, S, None, [sc.star_column(S, hub, [2, 3, 11000, 22000])], hub)


def similarRule(kind, ruleName, S):
    base = dict(ignoreValue=-7.0)
    if ruleName == 'threshold':
        base.update(maxDistance=6.0 if kind == 'star' else 1.0)
    elif ruleName == 'mutual':
        base.update(mutualNearest=True)
    else:
        base.update(mutualNearest=True, maxDistance=6.0 if kind == 'star' else 2.0, keyColumn=np.arange(S + 1) % 4 // 2,
                    ignoreKey=None if kind == 'star' else 1)
        if kind == 'star':
            base['keyColumn'] = np.zeros(S + 1, dtype=np.int64)
    return base


@functools.lru_cache(maxsize=None)
def oneGpuSimilar(kind, ruleName):
    (seg, S, size, cols, _hub) = similarInputs(kind)
    nb = neighbours.findSegmentNeighbours(seg, maxSegId=S)
    return neighbours.mergeSimilarSegments(nb, cols, segSize=size, segfile=seg, **similarRule(kind, ruleName, S))


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('ruleName', ['threshold', 'mutual', 'mutual_threshold_keys'])
@pytest.mark.parametrize('kind', ['drawn_large', 'A', 'star'])
def test_similar_merge_is_the_one_gpu_merge_on_every_rank(kind, ruleName, world):
    (seg, S, size, cols, hub) = similarInputs(kind)
    rule = similarRule(kind, ruleName, S)
    mutual = bool(rule.get('mutualNearest'))
    models = []

    def link(table):
        lm = sc.link_model(table, cols, maxDistance=rule.get('maxDistance'), mutualNearest=mutual, ignoreValue=-7.0,
                           keys=rule.get('keyColumn'), ignoreKey=rule.get('ignoreKey'), segSize=size)
        models.append((table, lm))
        return lm.link
    cuts = [0, 97, 300] if (kind == 'star' and world == 2) else cutsFor(seg.shape[0], world)
    ruleArgs = dict(distanceColumns=cols, segSize=size, **rule)
    (results, m) = checkAgainstOneGpuAndModel(seg, S, True, cuts, ruleArgs, oneGpuSimilar(kind, ruleName), link, size,
                                              mutual=mutual, what=(kind, ruleName, world))
    assert m['groups'].links > 0 and m['groups'].maxSegId < S
    if mutual:
        # ties in best across a share boundary: a row whose smallest d2 is held by candidates of different shares
        (table, lm) = models[0]
        (a, b, _w) = sc.entries(table)
        tied = np.flatnonzero(sc.ties_per_row(table, lm) >= 2)
        assert len(tied)
        bounds = np.array([distributed.idRange(r, world, S)[1] for r in range(world)])
        dmin = np.full(S + 1, np.inf)
        np.minimum.at(dmin, a[lm.candidate], lm.d2[lm.candidate])
        atMin = lm.candidate & (lm.d2 == dmin[a]) & np.isin(a, tied)
        owner = np.searchsorted(bounds, b[atMin], side='right')
        spread = {}
        for (row, o) in zip(a[atMin].tolist(), owner.tolist()):
            spread.setdefault(row, set()).add(o)
        assert any(len(v) >= 2 for v in spread.values()), (kind, world)
        if kind == 'star' and ruleName != 'mutual_threshold_keys':
            assert lm.best[hub] == 2 and len(spread[hub]) >= 2


# ---- two rounds -----------------------------------------------------------------------------------------------
def twoRoundInputs():
    (seg, S, keys, _emptyId, _base) = AC.raster()
    size = np.bincount(seg.ravel(), minlength=S + 1).astype(np.int64)
    vals = np.random.default_rng(31).random(S + 1) * 100.0
    return (seg, S, keys.astype(np.float64), size, vals)


def twoRounds(mergeSimilar, aggregate, reduce, first):
    """similar merge -> weighted mean of the groups -> its border mean -> merge again on the groups' table"""
    (_seg, _S, keysF, size, vals) = twoRoundInputs()
    m1 = mergeSimilar(first, [keysF], 0.5, size)
    agg = aggregate(m1, [(vals, [('wm', 'weightedmean'), ('n', 'count')])], size)
    red = reduce(m1.neighbours, [(agg['wm'], [('bm', 'bordermean'), ('near', 'nearest')])])
    m2 = mergeSimilar(m1.neighbours, [agg['wm']], 10.0, m1.hist)
    return (m1, agg, red, m2)


@functools.lru_cache(maxsize=None)
def oneGpuTwoRounds():
    (seg, S, _k, _size, _v) = twoRoundInputs()
    nb = neighbours.findSegmentNeighbours(seg, maxSegId=S)
    return twoRounds(lambda t, cols, dist, sz: neighbours.mergeSimilarSegments(t, cols, maxDistance=dist, segSize=sz),
                     lambda m, sel, w: neighbours.aggregateToGroups(m, sel, weights=w),
                     lambda t, sel: neighbours.reduceOverNeighbours(t, sel), nb)


@pytest.mark.parametrize('world', [2, 3])
def test_two_rounds_on_the_ranks_equal_two_rounds_on_one_gpu(world):
    (seg, S, _k, _size, _v) = twoRoundInputs()
    (w1, wagg, wred, w2) = oneGpuTwoRounds()
    assert {255, 256, 257} <= set(w1.groupSize.tolist()) and 0 < w2.maxSegId < w1.maxSegId and w2.links > 0
    cuts = {2: [0, 2, 4], 3: [0, 1, 2, 4]}[world]
    (nRows, nCols) = seg.shape

    def body(rank, comm, c):
        eng = types.SimpleNamespace(c=c)
        (lo, hi) = (cuts[rank], cuts[rank + 1])
        d = H.uploadRows(c, seg[lo:hi])
        try:
            share = distributed.deviceNeighbours(c, comm, d.value, nRows, nCols, (lo, hi), S)
            uploads = []

            def reduce(t, sel):
                out = distributed.reduceOverNeighboursDistributed(eng, comm, t, sel)
                uploads.append(t.reduceTimings['uploaded'])
                return out
            got = twoRounds(
                lambda t, cols, dist, sz: distributed.mergeSimilarSegmentsDistributed(eng, comm, t, cols, maxDistance=dist,
                                                                                       segSize=sz),
                lambda m, sel, w: distributed.aggregateToGroupsDistributed(eng, m, sel, weights=w), reduce, share)
            return got, uploads, got[0].aggregateTimings['uploaded']
        finally:
            c.check(c._L.shp_dev_free(c.handle, d))
    (results, errors) = H.runRankThreads(world, body)
    assert errors == [None] * world, errors
    for (rank, ((m1, agg, red, m2), uploads, aggUploaded)) in enumerate(results):
        assert uploads == [False] and aggUploaded is False
        for (got, want) in ((m1, w1), (m2, w2)):
            assertGroups(got, want, rank)
            assertShare(got, want.neighbours, rank, world, rank)
        for (got, want) in ((agg, wagg), (red, wred)):
            assert list(got) == list(want)
            for k in want:
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), k


def test_a_displaced_share_is_uploaded_again():
    (seg, S, size) = fieldA()
    want = oneGpuFieldA()
    cuts = H.cutsOf(2)
    small = NC.enclosed_by_zeros()
    keys = np.arange(S + 1) % 3

    def body(rank, comm, c):
        (lo, hi) = (cuts[rank], cuts[rank + 1])
        d = H.uploadRows(c, seg[lo:hi])
        d2 = H.uploadRows(c, small[20 * rank:20 * rank + 20])
        try:
            share = distributed.deviceNeighbours(c, comm, d.value, seg.shape[0], seg.shape[1], (lo, hi), S)
            distributed.deviceNeighbours(c, comm, d2.value, 40, small.shape[1], (20 * rank, 20 * rank + 20), 3)
            res = distributed.deviceMerge(c, comm, share, distributed.mergeRule(share, keys, segSize=size))
            again = distributed.reduceOverNeighboursDistributed(types.SimpleNamespace(c=c), comm, share,
                                                                [(size, [('b', 'border')])])
            return res, share.reduceTimings['uploaded'], again
        finally:
            for p in (d, d2):
                c.check(c._L.shp_dev_free(c.handle, p))
    (results, errors) = H.runRankThreads(2, body)
    assert errors == [None, None], errors
    for (rank, (res, reUploaded, _again)) in enumerate(results):
        assert res.timings['uploaded'] is True and reUploaded is True and res.outDev is None and res.rowRange is None
        assertGroups(res, want, rank)
        assertShare(res, want.neighbours, rank, 2, rank)


# ---- errors ---------------------------------------------------------------------------------------------------
def test_a_label_above_max_seg_id_on_one_rank_raises_on_every_rank():
    (seg, S, size) = fieldA()
    bad = seg.copy()
    cuts = H.cutsOf(3)
    bad[cuts[1] + 20, 7] = S + 20
    bad[cuts[1] + 31, 150] = S + 50
    (results, errors) = runMerge(seg, S, cuts, True, dict(keyColumn=np.arange(S + 1) % 3), mergeSeg=bad)
    assert results == [None] * 3
    for e in errors:
        assert isinstance(e, Err) and str(e) == 'segment id %d is above maxSegId %d' % (S + 50, S), errors


def test_overlapping_output_rows_raise_on_every_rank():
    (seg, S, size) = fieldA()
    (results, errors) = runMerge(seg, S, H.cutsOf(2), True, dict(keyColumn=np.arange(S + 1) % 3),
                                 mergeRanges=[(0, 120), (100, 203)])
    assert results == [None] * 2
    for e in errors:
        assert isinstance(e, Err) and 'SHEPSEG_SHARD=rows' in str(e), errors


def test_key_columns_of_different_length_raise_on_every_rank():
    (seg, S, size) = fieldA()
    cuts = H.cutsOf(2)

    def body(rank, comm, c):
        (lo, hi) = (cuts[rank], cuts[rank + 1])
        d = H.uploadRows(c, seg[lo:hi])
        try:
            share = distributed.deviceNeighbours(c, comm, d.value, seg.shape[0], seg.shape[1], (lo, hi), S)
            rule = distributed.mergeRule(share, np.arange(S + 1) % 3)
            if rank == 1:
                rule['keys'] = rule['keys'][:-1].copy()
            return distributed.deviceMerge(c, comm, share, rule)
        finally:
            c.check(c._L.shp_dev_free(c.handle, d))
    (results, errors) = H.runRankThreads(2, body)
    assert results == [None] * 2
    for e in errors:
        assert isinstance(e, Err) and 'different' in str(e), errors


def test_a_share_without_arrays_that_is_no_longer_resident_raises_on_every_rank():
    (seg, S, size) = fieldA()
    cuts = H.cutsOf(2)
    small = NC.enclosed_by_zeros()

    def body(rank, comm, c):
        (lo, hi) = (cuts[rank], cuts[rank + 1])
        d = H.uploadRows(c, seg[lo:hi])
        d2 = H.uploadRows(c, small[20 * rank:20 * rank + 20])
        try:
            share = distributed.deviceNeighbours(c, comm, d.value, seg.shape[0], seg.shape[1], (lo, hi), S,
                                                 fetch=rank == 1)
            distributed.deviceNeighbours(c, comm, d2.value, 40, small.shape[1], (20 * rank, 20 * rank + 20), 3)
            return distributed.deviceMerge(c, comm, share, distributed.mergeRule(share, np.arange(S + 1) % 3))
        finally:
            for p in (d, d2):
                c.check(c._L.shp_dev_free(c.handle, p))
    (results, errors) = H.runRankThreads(2, body)
    assert results == [None] * 2
    for e in errors:
        assert isinstance(e, Err) and 'no longer on the device' in str(e), errors


# ---- through the driver ---------------------------------------------------------------------------------------
def _runDriver(world, transport, tag, tmp_path, env=None):
    dist_cases.runRanks(world, [os.path.join(ROOT, 'tests', 'dist_worker_merge_gpu.py'), str(tmp_path), transport, tag],
                        tmp_path, 900, extra_env=env)


def _checkDriverRun(world, tmp_path, tag):
    base = str(tmp_path / tag)
    parts = [np.load('%s_rank%d.npz' % (base, r)) for r in range(world)]
    mosaic = np.load(base + '_labels.npy')
    S = int(parts[0]['maxSegId'])
    hist = parts[0]['hist']
    mean1 = parts[0]['mean1']
    dist = float(parts[0]['maxDistance'])
    whole = neighbours.findSegmentNeighbours(mosaic, maxSegId=S)
    want = neighbours.mergeSimilarSegments(whole, [mean1], maxDistance=dist, segSize=hist)
    agg = neighbours.aggregateToGroups(want, [(mean1, [('wm', 'weightedmean')])], weights=hist)
    red = neighbours.reduceOverNeighbours(want.neighbours, [(agg['wm'], [('bm', 'bordermean')])])
    M = want.maxSegId
    assert 0 < M < S and want.links > 0
    assert same(np.load(base + '_merged.npy'), want.recode[mosaic])
    for (r, q) in enumerate(parts):
        assert int(q['M']) == M and int(q['totalLinks']) == want.links and int(q['recordsSorted']) == want.recordsSorted
        for k in ('recode', 'representative', 'groupSize'):
            assert same(q[k], getattr(want, k)), (tag, r, k)
        assert same(q['newHist'], want.hist)
        (lo, hi) = distributed.idRange(r, world, M)
        assert (int(q['idLo']), int(q['idHi'])) == (lo, hi)
        (a, b) = (int(want.neighbours.offsets[lo]), int(want.neighbours.offsets[hi]))
        assert same(q['offsets'], want.neighbours.offsets[lo:hi + 1] - a)
        assert same(q['neighbours'], want.neighbours.neighbours[a:b])
        assert same(q['borderLengths'], want.neighbours.borderLengths[a:b])
        assert np.array_equal(q['wm'].view(np.uint64), agg['wm'].view(np.uint64))
        assert np.array_equal(q['bm'].view(np.uint64), red['bm'].view(np.uint64))
        assert not bool(q['reduceUploaded'])
    pairs = sum(int(q['forest_pairs']) for q in parts)
    sent = sum(int(q['records_sent']) for q in parts)
    for q in parts:
        assert int(q['exchange_bytes']) == 8 * pairs + 16 * sent
    print('%s: world %d, %d -> %d segments, %d links, %d pairs and %d records exchanged' % (tag, world, S, M, want.links,
                                                                                            pairs, sent))
    return parts


def test_through_the_driver_two_socket_ranks(tmp_path):
    """segmentation kept on the device -> table -> mean column -> similar merge with outfile -> aggregate -> reduction"""
    _runDriver(2, 'socket', 'rows', tmp_path, env={'SHEPSEG_SHARD': 'rows'})
    parts = _checkDriverRun(2, tmp_path, 'rows')
    assert sum(int(q['records_sent']) for q in parts) > 0 and all(int(q['forest_pairs']) > 0 for q in parts)


def test_through_the_driver_rccl_world_one(tmp_path):
    """the same pipeline with an RcclComm at world size 1 (the communicator on the device)"""
    _runDriver(1, 'rccl', 'rccl', tmp_path)
    parts = _checkDriverRun(1, tmp_path, 'rccl')
    assert int(parts[0]['records_sent']) == 0
