"""GPU: distributed.deviceMerge on id shares cut from hand-built tables (table_cases.share_of), in rank threads of one
process as test_gpu_merge_dist.py runs them, without label rows.  Every rank's groups against the numpy model, its new
share against the rows of the one-GPU result, its figures against the model of the split (merge_dist_cases).  The
tables are those of test_gpu_merge_tables.py: 64-bit lengths through the ranks' record exchange and the share merge's
partial sums, the refusal counted over all ranks, rows at the edges of the pieces of a share, and a graph whose groups
no rank holds whole."""
import functools
import types

import numpy as np
import pytest

import merge_cases as mc
import merge_dist_cases as MD
import stats_bands_dist_helpers as H
import table_cases as tc
from pyshepseg_amd import distributed, neighbours
from test_gpu_merge_dist import assertGroups, assertShare, same

pytestmark = pytest.mark.gpu
Err = neighbours.PyShepSegNeighboursError
WORLDS = [2, 3]


def runShares(table, world, ruleArgs, before=None, after=None):
    """deviceMerge without rows on share_of(table, rank, world) under mergeRule(share, **ruleArgs) in ``world`` rank
    threads; before / after(rank, comm, c[, res]): more work on the same context"""
    def body(rank, comm, c):
        first = before(rank, comm, c) if before else None
        share = tc.share_of(table, rank, world)
        info = {}
        res = distributed.deviceMerge(c, comm, share, distributed.mergeRule(share, **ruleArgs), info=info)
        return res, info, first, (after(rank, comm, c, res) if after else None)
    (results, errors) = H.runRankThreads(world, body)
    assert errors == [None] * world, errors
    return results


def checkRanks(results, split, oneGpu, hist=False):
    """every rank against the model of the split and, with ``oneGpu``, against the one-GPU result"""
    world = len(results)
    for (rank, (res, info, _first, _more)) in enumerate(results):
        assertGroups(res, split['groups'], ('model', rank), hist=hist)
        want = split['ranks'][rank]
        assert res.neighbours.idRange == want['idRange'] and res.outDev is None and res.rowRange is None
        for k in ('offsets', 'neighbours', 'borderLengths'):
            assert same(getattr(res.neighbours, k), want[k]), (rank, k)
        if oneGpu is not None:
            assertGroups(res, oneGpu, ('one GPU', rank), hist=hist)
            assertShare(res, oneGpu.neighbours, rank, world, rank)
        info = dict(info)
        info.pop('deviceMs')
        assert info == MD.info_of(split, rank), (rank, info, MD.info_of(split, rank))


@functools.lru_cache(maxsize=None)
def wide():
    (table, keys) = tc.wide_sums()
    return (table, keys, neighbours.mergeSegments(tc.whole_of(table), keys))


WIDE_COLUMN = np.array([0, 3, -2, 5, 1, -7, 4, 2, -1, 6, -3, 8, -5], dtype=np.float64)
WIDE_STATS = [(WIDE_COLUMN, [('b', 'border'), ('bm', 'bordermean')])]


@pytest.mark.parametrize('world', WORLDS)
def test_wide_sums_on_the_ranks_and_their_reduction(world):
    (table, keys, oneGpu) = wide()
    split = MD.model(table, MD.key_links(table, keys), world)
    assert sum(r['records_sent'] for r in split['ranks']) > 0 and int((split['groups'].table[2] >= tc.TWO32).sum()) == 22

    def reduce(rank, comm, c, res):
        out = distributed.reduceOverNeighboursDistributed(types.SimpleNamespace(c=c), comm, res.neighbours, WIDE_STATS)
        return out, res.neighbours.reduceTimings['uploaded']
    results = runShares(table, world, dict(keyColumn=keys), after=reduce)
    checkRanks(results, split, oneGpu)
    want = neighbours.reduceOverNeighbours(oneGpu.neighbours, WIDE_STATS)
    row = np.repeat(np.arange(tc.GROUPS + 1), np.diff(oneGpu.neighbours.offsets))
    exact = [sum(oneGpu.neighbours.borderLengths[row == g].tolist()) for g in range(tc.GROUPS + 1)]     # (Python integers)
    assert want['b'].tolist() == exact and min(exact[1:]) >= tc.TWO32
    for (rank, (_res, _info, _first, (out, uploaded))) in enumerate(results):
        assert uploaded is False and list(out) == list(want)
        for k in want:
            assert same(out[k], want[k]), (rank, k)


@pytest.mark.parametrize('world', WORLDS)
def test_piece_geometry_on_the_ranks(world):
    g = tc.piece_geometry(4096)
    oneGpu = neighbours.mergeSegments(tc.whole_of(g.table), g.keys, segSize=g.segSize)
    split = MD.model(g.table, MD.key_links(g.table, g.keys, segSize=g.segSize), world, g.segSize)
    results = runShares(g.table, world, dict(keyColumn=g.keys, segSize=g.segSize))
    checkRanks(results, split, oneGpu, hist=True)
    assert sum(r['links'] for r in split['ranks']) == oneGpu.links > 0


@pytest.mark.parametrize('world', WORLDS)
def test_wide_refused_on_every_rank_and_the_contexts_go_on(world):
    (good, keys, oneGpu) = wide()
    (bad, _keys, at) = tc.wide_refused('2^32')
    owners = {int(np.searchsorted([distributed.idRange(r, world, tc.WIDE_S)[1] for r in range(world)], a, side='right'))
              for a in np.repeat(np.arange(tc.WIDE_S + 1), np.diff(bad[0]))[at]}
    assert len(owners) >= 2                     # (the three entries are counted on different ranks and added up)

    def refused(rank, comm, c):
        share = tc.share_of(bad, rank, world)
        try:
            distributed.deviceMerge(c, comm, share, distributed.mergeRule(share, keyColumn=keys))
        except Err as e:
            return str(e)
        return None
    results = runShares(good, world, dict(keyColumn=keys), before=refused)
    message = ("{} border lengths of the table are outside 1 .. 2^32 - 1: the contraction's records hold 32-bit "
               "lengths".format(len(at)))
    assert [r[2] for r in results] == [message] * world
    checkRanks(results, MD.model(good, MD.key_links(good, keys), world), oneGpu)


def test_random_graph_groups_no_rank_holds_whole():
    table = tc.random_graph()
    keys = tc.class_keys(len(table[0]) - 2, 2)
    split = MD.model(table, MD.key_links(table, keys), 3)
    assert MD.groups_no_rank_holds_whole(split) >= 1
    results = runShares(table, 3, dict(keyColumn=keys))
    checkRanks(results, split, None)
    model = mc.reference_merge(table, keys)
    for (res, _info, _first, _more) in results:
        assertGroups(res, model, 'reference_merge', hist=False)
