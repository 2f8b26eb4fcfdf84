"""GPU: mergeSegments, mergeSimilarSegments, the contraction, reduceOverNeighbours on the contracted table and
aggregateToGroups on neighbour tables built by hand (tests/table_cases.py), against the numpy definitions the raster
cases use (merge_cases, similar_cases, aggregate_cases, neighbour_reduce_cases).  A hand-built table reaches what no
raster of test size does: contracted lengths of 2^32 and more and the refusal of a length no record holds, rows at
the edges of the hook's pieces, graphs that are not planar, and ids, members and labels beyond the first trip of the
grid-stride loops.  Everything is compared with numpy.array_equal and its dtype; tests/test_table_cases_host.py
asserts from the models that every case reaches what it is here for."""
import functools
import re

import numpy as np
import pytest

import aggregate_cases as ac
import merge_cases as mc
import neighbour_reduce_cases as rc
import similar_cases as sc
import table_cases as tc
from test_gpu_merge import assert_groups

pytestmark = pytest.mark.gpu


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


@functools.lru_cache(maxsize=None)
def wide():
    """(table, keys, the model's groups): computed once, shared, left unchanged"""
    (table, keys) = tc.wide_sums()
    return (table, keys, mc.reference_merge(table, keys))


def refusal(count):
    return re.escape('{} border lengths outside 1 .. 2^32 - 1'.format(count))


def upload_refusal(table):
    """what the upload's check says of a table with lengths below 1: it names the first of them"""
    return re.escape('not a neighbour table: entry {}: a border length below 1'.format(int(np.flatnonzero(table[2] < 1)[0])))


# ---- sums of 32-bit record lengths past 2^32 ------------------------------------------------------------------
def test_wide_sums_through_both_rules_and_the_reduction():
    from pyshepseg_amd import neighbours
    (table, keys, model) = wide()
    assert int((model.table[2] >= tc.TWO32).sum()) == 22
    res = neighbours.mergeSegments(tc.whole_of(table), keys)
    assert res.timings['uploaded'] is True
    assert_groups(res, model)
    similar = sc.reference_similar(table, [keys], maxDistance=0)
    for (got, want) in zip(similar.table, model.table):
        same(got, want, 'the two models')
    res = neighbours.mergeSimilarSegments(tc.whole_of(table), [keys.astype(np.int32)], maxDistance=0)
    assert_groups(res, similar)
    # the contracted table, still on the device, reduced: its lengths are read as 64-bit integers
    column = np.array([0, 3, -2, 5, 1, -7, 4, 2, -1, 6, -3, 8, -5], dtype=np.int64)
    stats = ('border', 'count', 'bordermean', 'mean')
    out = neighbours.reduceOverNeighbours(res.neighbours, [(column, [(s, s) for s in stats])])
    assert res.neighbours.reduceTimings['uploaded'] is False
    want = rc.reference_reduce(*model.table, column, stats=stats)
    for s in stats:
        same(out[s], want[s], s)
    (a, _b, w) = sc.entries(model.table)
    exact = [sum(w[a == g].tolist()) for g in range(tc.GROUPS + 1)]                  # (Python integers)
    assert out['border'].tolist() == exact and min(exact[1:]) >= tc.TWO32


@pytest.mark.parametrize('kind', list(tc.REFUSED))
def test_wide_refused_and_the_context_goes_on(kind):
    """three lengths no record holds between two groups; then the good table on the same context; then the same
    lengths inside a group, where no record is made of them.  A length below 1 is no neighbour table wherever it
    lies: the upload's check refuses it before the merge sees it, and names the first such entry."""
    from pyshepseg_amd import _lib, neighbours
    (good, keys, model) = wide()
    (table, _keys, at) = tc.wide_refused(kind)
    if tc.REFUSED[kind] >= 1:
        with pytest.raises(_lib.ShepsegHipError, match=refusal(len(at))):
            neighbours.mergeSegments(tc.whole_of(table), keys)
        with pytest.raises(_lib.ShepsegHipError, match=refusal(len(at))):
            neighbours.mergeSimilarSegments(tc.whole_of(table), [keys], maxDistance=0)
    else:
        with pytest.raises(neighbours.PyShepSegNeighboursError, match=upload_refusal(table)):
            neighbours.mergeSegments(tc.whole_of(table), keys)
    assert_groups(neighbours.mergeSegments(tc.whole_of(good), keys), model)
    (inside, _keys, at) = tc.wide_refused(kind, between=False)
    if tc.REFUSED[kind] >= 1:
        assert_groups(neighbours.mergeSegments(tc.whole_of(inside), keys), model)
    else:
        with pytest.raises(neighbours.PyShepSegNeighboursError, match=upload_refusal(inside)):
            neighbours.mergeSegments(tc.whole_of(inside), keys)
        assert_groups(neighbours.mergeSegments(tc.whole_of(good), keys), model)


def test_wide_inside_groups_and_min_border():
    from pyshepseg_amd import _lib, neighbours
    (table, keys) = tc.wide_inside_groups()
    at1 = mc.reference_merge(table, keys)
    assert_groups(neighbours.mergeSegments(tc.whole_of(table), keys), at1)
    at40 = mc.reference_merge(table, keys, minBorder=tc.INSIDE_40)
    res = neighbours.mergeSegments(tc.whole_of(table), keys, minBorder=tc.INSIDE_40)
    assert_groups(res, at40)
    assert res.links == 2 * tc.GROUPS * 275 < at1.links and res.maxSegId > at1.maxSegId
    # one above: the 2^40 entries link no more, lie between two groups, and no record holds them
    above = mc.reference_merge(table, keys, minBorder=tc.INSIDE_40 + 1)
    assert above.links == tc.GROUPS * 275
    with pytest.raises(_lib.ShepsegHipError, match=refusal(tc.GROUPS * 275)):
        neighbours.mergeSegments(tc.whole_of(table), keys, minBorder=tc.INSIDE_40 + 1)


# ---- rows at the edges of the pieces --------------------------------------------------------------------------
@pytest.mark.parametrize('nent', tc.NENTS)
def test_piece_geometry_key_rule(nent):
    from pyshepseg_amd import neighbours
    g = tc.piece_geometry(nent)
    model = mc.reference_merge(g.table, g.keys, segSize=g.segSize)
    res = neighbours.mergeSegments(tc.whole_of(g.table), g.keys, segSize=g.segSize)
    assert_groups(res, model)
    same(res.hist, model.hist, 'hist')
    assert 0 < res.links < len(g.leaves) and res.recordsSorted == len(g.leaves) - res.links


@pytest.mark.parametrize('nent', tc.NENTS)
def test_piece_geometry_mutual_rule(nent):
    from pyshepseg_amd import neighbours
    g = tc.piece_geometry(nent)
    model = sc.reference_similar(g.table, [g.column], mutualNearest=True, segSize=g.segSize)
    res = neighbours.mergeSimilarSegments(tc.whole_of(g.table), [g.column], mutualNearest=True, segSize=g.segSize)
    assert_groups(res, model)
    assert res.links == len(g.hubs)
    want = g.first if g.flip else g.last
    assert np.array_equal(res.recode[g.hubs], res.recode[want])
    # the threshold rule over the same rows: every near leaf, and the key rule on top of it
    model = sc.reference_similar(g.table, [g.column], maxDistance=5, keys=g.keys, segSize=g.segSize)
    res = neighbours.mergeSimilarSegments(tc.whole_of(g.table), [g.column], maxDistance=5, keyColumn=g.keys, segSize=g.segSize)
    assert_groups(res, model)


# ---- graphs that are not planar -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph():
    return tc.random_graph()


@pytest.mark.parametrize('classes', [1, 2, 50])
def test_random_graph(classes):
    from pyshepseg_amd import neighbours
    table = graph()
    keys = tc.class_keys(len(table[0]) - 2, classes)
    model = mc.reference_merge(table, keys)
    res = neighbours.mergeSegments(tc.whole_of(table), keys)
    assert_groups(res, model)
    assert res.links == model.links > 3000 and res.recordsSorted == model.recordsSorted
    res = neighbours.mergeSimilarSegments(tc.whole_of(table), [keys], maxDistance=0.5)
    assert_groups(res, sc.reference_similar(table, [keys], maxDistance=0.5))
    assert res.links == model.links


@pytest.mark.parametrize('name', ['complete_bipartite', 'folded_chain'])
def test_one_root_under_many_hooks(name):
    from pyshepseg_amd import neighbours
    (table, keys) = getattr(tc, name)()
    model = mc.reference_merge(table, keys)
    res = neighbours.mergeSegments(tc.whole_of(table), keys)
    assert_groups(res, model)
    assert res.maxSegId == 1 and res.links == len(table[1]) // 2 and res.recordsSorted == 0
    assert res.representative.tolist() == [0, 1] and res.groupSize.tolist() == [0, len(table[0]) - 2]


# ---- ids and members beyond the first trip of a launch of 2048 workgroups -------------------------------------
def test_sparse_wide_merge_and_aggregate():
    from pyshepseg_amd import neighbours
    s = tc.sparse_wide()
    S = tc.SPARSE_S
    model = sc.reference_similar(s.table, s.columns, maxDistance=s.maxDistance, ignoreValue=s.ignoreValue)
    res = neighbours.mergeSimilarSegments(tc.whole_of(s.table), s.columns, maxDistance=s.maxDistance,
                                          ignoreValue=s.ignoreValue)
    assert_groups(res, model)
    assert res.groupSize[res.recode[s.hole]] == 1 and (res.groupSize[res.recode[s.high]] > 1).sum() > 20
    rng = np.random.default_rng(601)
    weights = 1 + np.arange(S + 1, dtype=np.int64) % 5
    f32 = rng.integers(0, 10, size=S + 1).astype(np.float32)
    i64 = rng.integers(-50, 51, size=S + 1).astype(np.int64)
    f64 = rng.integers(-9, 10, size=S + 1).astype(np.float64)
    selections = [(f32, [('f32mean', 'mean'), ('f32max', 'max')]),
                  (i64, [('isum', 'sum'), ('imin', 'min'), ('imean', 'mean')]),
                  (f64, [('wm', 'weightedmean'), ('fsum', 'sum'), ('w', 'weight'), ('n', 'count')])]
    names = {'f32mean': (f32, 'mean'), 'f32max': (f32, 'max'), 'isum': (i64, 'sum'), 'imin': (i64, 'min'),
             'imean': (i64, 'mean'), 'wm': (f64, 'weightedmean'), 'fsum': (f64, 'sum'), 'w': (f64, 'weight'),
             'n': (f64, 'count')}
    for w in (weights, None, weights[::-1].copy()):
        out = neighbours.aggregateToGroups(res, selections, weights=w)
        refs = {id(col): ac.reference_aggregate(model.recode, model.maxSegId, col, weights=w) for col in (f32, i64, f64)}
        for (name, (col, stat)) in names.items():
            same(out[name], refs[id(col)][stat], (name, w is None))
        assert out['isum'].dtype == np.int64
    # without segSize every id is a vertex: the member list holds them all
    assert len(res.membersOf(res.maxSegId)) >= 1 and len(res.members) == S > tc.ONE_TRIP
    (offsets, members) = ac.member_csr(model.recode, model.maxSegId)
    same(res.memberOffsets, offsets, 'memberOffsets')
    same(res.members, members, 'members')
    # the mutual rule over the same columns (its two per-id arrays are filled beyond the first trip as well)
    model = sc.reference_similar(s.table, s.columns, mutualNearest=True, ignoreValue=s.ignoreValue)
    res = neighbours.mergeSimilarSegments(tc.whole_of(s.table), s.columns, mutualNearest=True, ignoreValue=s.ignoreValue)
    assert_groups(res, model)


# ---- more labels than one trip of the recode ------------------------------------------------------------------
def test_recode_of_a_raster_larger_than_one_trip():
    from pyshepseg_amd import neighbours
    case = [c for c in mc.CASES if c.name == 'drawn_large'][0]
    (_seg, S, keys, _size, table) = mc.build(case, True)
    big = tc.large_raster(S)
    assert big.size > tc.RECODE_ONE_TRIP
    model = mc.reference_merge(table, keys)
    want = model.recode[big]
    hist = np.bincount(want.ravel(), minlength=model.maxSegId + 1).astype(np.int64)
    assert 1 < model.maxSegId < S
    # the histogram counted in the pass, in one block and in two (1050 rows, then 50)
    for chunk in (None, tc.RECODE_BLOCK_ROWS * big.shape[1]):
        res = neighbours.mergeSegments(tc.whole_of(table), keys, segfile=big, chunkPixels=chunk)
        assert_groups(res, model)
        same(res.segimg, want, ('segimg', chunk))
        same(res.hist, hist, ('hist', chunk))
    # the histogram from segSize
    size = np.bincount(big.ravel(), minlength=S + 1).astype(np.int64)
    sized = mc.reference_merge(table, keys, segSize=size)
    res = neighbours.mergeSegments(tc.whole_of(table), keys, segSize=size, segfile=big)
    assert_groups(res, sized)
    same(res.segimg, sized.recode[big], 'segimg with segSize')
    same(res.hist, sized.hist, 'hist with segSize')
    assert np.array_equal(res.hist, np.bincount(res.segimg.ravel(), minlength=res.maxSegId + 1))
