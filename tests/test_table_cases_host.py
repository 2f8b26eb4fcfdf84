"""CPU: the hand-built tables of tests/table_cases.py are what they claim to be.  Every table is a neighbour table
(symmetric, ascending rows, arrays of the lengths of its S); every claim about where rows fall in the hook's pieces is
read from the offsets; every claim about what a case reaches (sums past 2^32, links and non-links, groups no rank
holds) is read from the models, so that no GPU case of test_gpu_merge_tables*.py passes empty."""
import functools

import numpy as np
import pytest

import merge_cases as mc
import merge_dist_cases as MD
import neighbour_reduce_cases as rc
import similar_cases as sc
import table_cases as tc

PIECE = tc.PIECE


def assert_is_table(table, dangling=None):
    (offsets, nbrs, lens) = table
    S = len(offsets) - 2
    assert offsets.dtype == np.int64 and nbrs.dtype == np.uint32 and lens.dtype == np.int64
    assert len(nbrs) == len(lens) == offsets[-1]
    assert 'length' not in rc.table_violations(offsets, nbrs, np.maximum(lens, 1))
    assert [v for v in rc.table_violations(offsets, nbrs, lens) if v != 'length'] == []
    (a, b, w) = sc.entries(table)
    if dangling is not None:
        assert (int(a[-1]), int(b[-1])) == dangling
        (a, b, w) = (a[:-1], b[:-1], w[:-1])
    # every pair from both sides with one length: the entries sorted by (a, b) are the entries sorted by (b, a)
    (fwd, back) = (np.lexsort((b, a)), np.lexsort((a, b)))
    assert np.array_equal(a[fwd], b[back]) and np.array_equal(b[fwd], a[back]) and np.array_equal(w[fwd], w[back])
    return S


def bound_of_sums(table):
    """an upper bound of every sum of lengths the contraction can form: all entries a < b together"""
    (_a, _b, w, _e) = tc.edges_of(table)
    return float(np.abs(w.astype(np.float64)).sum())


@functools.lru_cache(maxsize=None)
def wide():
    (table, keys) = tc.wide_sums()
    return (table, keys, mc.reference_merge(table, keys))


# ---- the helpers ----------------------------------------------------------------------------------------------
def test_table_from_edges_by_hand():
    (offsets, nbrs, lens) = tc.table_from_edges(5, [1, 1, 3], [4, 2, 4], [7, 1 << 40, 9])
    assert offsets.tolist() == [0, 0, 2, 3, 4, 6, 6] and nbrs.tolist() == [2, 4, 1, 4, 1, 3]
    assert lens.tolist() == [1 << 40, 7, 1 << 40, 9, 7, 9]
    assert (offsets.dtype, nbrs.dtype, lens.dtype) == (np.int64, np.uint32, np.int64)
    with pytest.raises(AssertionError):
        tc.table_from_edges(5, [1, 1], [4, 4], [1, 1])


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('name', ['wide_sums', 'piece_geometry', 'random_graph'])
def test_shares_assemble_to_the_table(name, world):
    from pyshepseg_amd import distributed
    table = {'wide_sums': lambda: wide()[0], 'piece_geometry': lambda: tc.piece_geometry(4096).table,
             'random_graph': lambda: tc.random_graph(2000, 4, 3)}[name]()
    S = len(table[0]) - 2
    shares = [tc.share_of(table, r, world) for r in range(world)]
    whole = tc.whole_of(table).columns
    for (r, sh) in enumerate(shares):
        assert sh.idRange == distributed.idRange(r, world, S) and sh.maxSegId == S
        assert len(sh.offsets) == sh.idRange[1] - sh.idRange[0] + 1 and sh.offsets[0] == 0
        for k in ('numNeighbours', 'borderLength'):
            assert sh.columns[k].dtype == np.int64 and np.array_equal(sh.columns[k], whole[k])
    ranks = [dict(idRange=sh.idRange, offsets=sh.offsets, neighbours=sh.neighbours, borderLengths=sh.borderLengths)
             for sh in shares]
    for (got, want) in zip(MD.assembled(ranks, S), table):
        assert got.dtype == want.dtype and np.array_equal(got, want)


# ---- sums past 2^32 ---------------------------------------------------------------------------------------------
def test_wide_sums_reach_the_carry():
    (table, keys, m) = wide()
    assert assert_is_table(table) == tc.WIDE_S == 13200
    assert len(table[1]) == 2 * (tc.GROUPS * (tc.MEMBERS - 1) + sum(tc.MULT)) == 30820
    assert m.maxSegId == tc.GROUPS and m.groupSize[1:].tolist() == [tc.MEMBERS] * tc.GROUPS
    assert m.recordsSorted == sum(tc.MULT) == 2222 and m.links == tc.GROUPS * (tc.MEMBERS - 1)
    # the records of a pair of groups: runs inside a wavefront, across wavefronts, across workgroups of 256 records
    (a, b, w, _e) = tc.edges_of(table)
    (ra, rb) = (m.recode[a].astype(np.int64), m.recode[b].astype(np.int64))
    cross = ra != rb
    runs = np.bincount(np.minimum(ra, rb)[cross] * 100 + np.maximum(ra, rb)[cross])
    assert sorted(runs[runs > 0].tolist()) == sorted(tc.MULT) and runs.max() > 256
    assert w[cross].min() >= 1 and w[cross].max() == tc.TWO32 - 1 and (w[~cross] == 1).all()
    # the contracted lengths: exact in Python integers, 22 of 24 at or above 2^32, all far below 2^63
    exact = {}
    for (x, y, v) in zip(np.minimum(ra, rb)[cross].tolist(), np.maximum(ra, rb)[cross].tolist(), w[cross].tolist()):
        exact[(x, y)] = exact.get((x, y), 0) + v
    (offsets, nbrs, lens) = m.table
    assert len(nbrs) == 24 and int((lens >= tc.TWO32).sum()) == 22
    rows = np.repeat(np.arange(tc.GROUPS + 1), np.diff(offsets))
    for (r, n, v) in zip(rows.tolist(), nbrs.tolist(), lens.tolist()):
        assert exact[(min(r, n), max(r, n))] == v
    assert max(exact.values()) == int(lens.max()) > 1000 * (1 << 31) and bound_of_sums(table) < 2.0 ** 62
    print('wide_sums: %d entries, %d pieces, %d groups, %d records, largest contracted length %d'
          % (len(table[1]), -(-len(table[1]) // PIECE), m.maxSegId, m.recordsSorted, int(lens.max())))


@pytest.mark.parametrize('world', [2, 3])
def test_wide_sums_records_travel_and_stay_home(world):
    (table, keys, m) = wide()
    split = MD.model(table, MD.key_links(table, keys), world)
    assert sum(r['records_sent'] for r in split['ranks']) > 0 and sum(r['records_home'] for r in split['ranks']) > 0
    assert sum(r['records_entries'] for r in split['ranks']) == m.recordsSorted
    assert all(r['forest_pairs'] > 0 for r in split['ranks'])


@pytest.mark.parametrize('kind', list(tc.REFUSED))
@pytest.mark.parametrize('between', [True, False], ids=['between', 'inside'])
def test_wide_refused_replaces_three_lengths(kind, between):
    (good, keys, m) = wide()
    (table, keys2, at) = tc.wide_refused(kind, between)
    assert np.array_equal(keys, keys2) and np.array_equal(table[0], good[0]) and np.array_equal(table[1], good[1])
    assert_is_table(table)
    changed = np.flatnonzero(table[2] != good[2])
    assert len(changed) == 6 and (table[2][changed] == tc.REFUSED[kind]).all() and set(at.tolist()) < set(changed.tolist())
    (a, b, _w) = sc.entries(table)
    assert (a[at] < b[at]).all() and ((m.recode[a[changed]] != m.recode[b[changed]]) == between).all()
    pieces = at // PIECE
    assert pieces[0] == 0 and pieces[-1] == (len(table[1]) - 1) // PIECE and 0 < pieces[1] < pieces[-1]
    # what the upload's check names first: the first entry below 1, from whichever side
    if tc.REFUSED[kind] < 1:
        assert changed[0] <= at[0] and 'length' in rc.table_violations(*table)
    else:
        assert rc.table_violations(*table) == []


def test_wide_inside_groups_by_the_model():
    (table, keys) = tc.wide_inside_groups()
    assert_is_table(table)
    (a, b, w, _e) = tc.edges_of(table)
    (n62, n40) = (int((w == tc.INSIDE_62).sum()), int((w == tc.INSIDE_40).sum()))
    assert n62 == tc.GROUPS * 275 and n40 == tc.GROUPS * 275 and (np.sort(np.unique(w))[-2:] == [tc.INSIDE_40, tc.INSIDE_62]).all()
    # a row's lengths sum below 2^63 (the share's borderLength column)
    assert tc.columns_of(table)['borderLength'].max() < tc.INSIDE_62 + tc.INSIDE_40 + 3000 and bound_of_sums(table) > 2.0 ** 63
    at1 = mc.reference_merge(table, keys)
    assert at1.maxSegId == tc.GROUPS and (at1.recode[a] == at1.recode[b])[w >= tc.INSIDE_40].all()
    assert at1.recordsSorted == sum(tc.MULT) and at1.table[2].max() < 1000 * 1000
    at40 = mc.reference_merge(table, keys, minBorder=tc.INSIDE_40)
    assert at40.links == n62 + n40 and at40.table[2].max() < 1000 * 1000 and set(at40.groupSize[1:].tolist()) == {2}
    above = mc.reference_merge(table, keys, minBorder=tc.INSIDE_40 + 1)
    assert above.links == n62
    # one step above, the 2^40 entries lie between two groups: the contraction must refuse them, all of them
    assert int(((above.recode[a] != above.recode[b]) & (w == tc.INSIDE_40)).sum()) == n40


# ---- rows at the edges of the pieces ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometry(nent):
    g = tc.piece_geometry(nent)
    g.keyLink = MD.key_links(g.table, g.keys, segSize=g.segSize)
    g.keyModel = mc.reference_merge(g.table, g.keys, segSize=g.segSize)
    g.mutualModel = sc.reference_similar(g.table, [g.column], mutualNearest=True, segSize=g.segSize)
    return g


def claims_of(g):
    """{(claim, link on the entry at the edge)} read from the offsets; the link is the key rule's"""
    offsets = g.table[0]
    S = len(offsets) - 2
    rows = np.flatnonzero(np.diff(offsets))
    found = set()
    for (i, r) in enumerate(rows.tolist()):
        (x, y) = (int(offsets[r]), int(offsets[r + 1]))
        if y % PIECE == 0:
            found.add(('row ends on the last entry of a piece', bool(g.keyLink[y - 1])))
        if x % PIECE == 0 and y - x == PIECE:
            found.add(('row is exactly one piece', bool(g.keyLink[y - 1])))
        if x % PIECE == PIECE - 1:
            found.add(('row starts on the last entry of a piece', bool(g.keyLink[x])))
        if i > 0 and x % PIECE == 0 and r - rows[i - 1] - 1 >= 3000:
            found.add(('3000 empty rows where a piece ends', bool(g.keyLink[x - 1])))
    if rows[0] - 1 >= 3000:
        found.add(('3000 empty rows in front', bool(g.keyLink[0])))
    if rows[-1] < S:
        found.add(('empty rows behind', bool(g.keyLink[-1])))
    return found


def test_piece_geometry_claims():
    assert tc.NENTS == [2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145] == sorted(tc.GEOMETRY)
    found = set()
    for nent in tc.NENTS:
        g = geometry(nent)
        S = assert_is_table(g.table, g.dangling)
        assert len(g.table[1]) == nent and len(g.keys) == len(g.column) == len(g.segSize) == S + 1
        assert (g.dangling is not None) == (nent % 2 == 1)
        if g.dangling:
            (a, b) = g.dangling
            assert a < b and g.segSize[b] == 0 and g.table[0][b] == g.table[0][b + 1] and int(g.segSize.sum()) == S
            assert not g.keyLink[-1] and g.keyModel.recode[b] == 0
        found |= claims_of(g)
        # the hubs' rows are read by the hook (a < b), the leaves' by the mutual rule alone; both link and not
        (a, b, _w) = sc.entries(g.table)
        assert g.keyLink[a < b].any() and (~g.keyLink[a < b]).any()
        assert np.array_equal(np.unique(g.keys[g.leaves]), [0, 1]) and (np.diff(g.keys[g.leaves]) != 0).all()
    assert geometry(2049).table[0][-1] - 1 == PIECE         # (the dangling entry is alone in the last piece)
    claims = {c for (c, _link) in found}
    assert len(claims) == 6
    missing = [(c, link) for c in sorted(claims) for link in (True, False) if (c, link) not in found]
    assert missing == [], missing


def test_piece_geometry_mutual_rule_is_decided_across_pieces():
    split = 0
    for nent in tc.NENTS:
        g = geometry(nent)
        m = g.mutualModel
        want = g.first if g.flip else g.last
        assert np.array_equal(m.rule.best[g.hubs], want) and m.links == len(g.hubs)
        assert (m.rule.candidate & ~m.rule.link).any() and set(m.groupSize[1:].tolist()) == {1, 2}
        (offsets, nbrs, _lens) = g.table
        for (h, f, l) in zip(g.hubs.tolist(), g.first.tolist(), g.last.tolist()):
            (x, y) = (int(offsets[h]), int(offsets[h + 1]))
            assert (int(nbrs[x]), int(nbrs[y - 1])) == (f, l)
            ties = sc.ties_per_row(g.table, m.rule)[h]
            assert ties == (2 if g.flip and f != l else 1)
            if ties == 2 and x // PIECE != (y - 1) // PIECE:
                split += 1
                assert x % PIECE == PIECE - 1           # the winner of the tie is the last entry of its piece
    assert split >= 1
    # and a best that lies in the piece behind the one the row starts in, without a tie
    g = geometry(6143)
    (x, y) = (int(g.table[0][g.hubs[1]]), int(g.table[0][g.hubs[1] + 1]))
    assert x // PIECE == 0 and (y - 1) // PIECE == 1 and not g.flip


# ---- graphs -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph():
    return tc.random_graph()


@pytest.mark.parametrize('classes,groups,records', [(1, (1, 1), (0, 0)), (2, (2, 20), (70000, 90000)),
                                                    (50, (15000, 18500), (150000, 160000))])
def test_random_graph_reach(classes, groups, records):
    table = graph()
    S = assert_is_table(table)
    assert S == 20000 and 310000 < len(table[1]) < 320001 and len(table[1]) // PIECE > 150
    keys = tc.class_keys(S, classes)
    m = mc.reference_merge(table, keys)
    assert groups[0] <= m.maxSegId <= groups[1] and records[0] <= m.recordsSorted <= records[1]
    assert m.links + m.recordsSorted == len(table[1]) // 2 and m.links > 0
    assert bound_of_sums(table) < 2.0 ** 40
    print('random_graph/%d: %d entries, %d pieces, %d groups, %d links, %d records, largest contracted length %d'
          % (classes, len(table[1]), -(-len(table[1]) // PIECE), m.maxSegId, m.links, m.recordsSorted,
             int(m.table[2].max()) if len(m.table[2]) else 0))


def test_random_graph_groups_no_rank_holds_whole():
    table = graph()
    keys = tc.class_keys(20000, 2)
    split = MD.model(table, MD.key_links(table, keys), 3)
    assert MD.groups_no_rank_holds_whole(split) >= 1


def test_complete_bipartite_and_folded_chain_reach():
    (table, keys) = tc.complete_bipartite(300)
    assert assert_is_table(table) == 600 and len(table[1]) == 180000
    m = mc.reference_merge(table, keys)
    assert (m.maxSegId, m.links, m.recordsSorted) == (1, 90000, 0) and m.representative.tolist() == [0, 1]
    (table, keys) = tc.folded_chain()
    assert assert_is_table(table) == 20000
    m = mc.reference_merge(table, keys)
    (a, b, _w, _e) = tc.edges_of(table)
    assert (m.maxSegId, m.recordsSorted) == (1, 0) and m.links == len(a) == 19999 + 9999
    assert ((b - a == 1).sum(), (a + b == 20001).sum()) == (19999, 10000)       # (10000, 10001) is both


# ---- ids past one trip ------------------------------------------------------------------------------------------
def test_sparse_wide_reach():
    s = tc.sparse_wide()
    S = assert_is_table(s.table)
    assert S == tc.SPARSE_S == 600000 and tc.ONE_TRIP == 524288
    (a, b, _w) = sc.entries(s.table)
    low = a <= 5000
    assert 3000 < low.sum() < 4100 and (b[low] <= 5000).all()
    assert 400 < (~low).sum() < 601 and (a[~low] > tc.ONE_TRIP).all() and (b[~low] > tc.ONE_TRIP).all()
    assert np.isin(a[~low], s.high).all() and int((np.diff(s.table[0]) == 0).sum()) > S - 5200
    assert [c.dtype for c in s.columns] == [np.float64, np.float32, np.int16]
    m = sc.reference_similar(s.table, s.columns, maxDistance=s.maxDistance, ignoreValue=s.ignoreValue)
    link = m.rule.link
    assert (link & ~low).any() and (m.rule.candidate & ~link & ~low).any(), 'links and non-links among the high ids'
    assert (link & low).any() and (m.rule.candidate & ~link & low).any()
    # the hole: a high id, the only id with the ignore value, alone in its group; it links once the value is filled
    bad = np.flatnonzero(sc.ignored_ids(s.columns, s.ignoreValue))
    assert bad.tolist() == [s.hole] and s.hole > tc.ONE_TRIP and m.groupSize[m.recode[s.hole]] == 1
    filled = sc.reference_similar(s.table, s.holeFilled, maxDistance=s.maxDistance, ignoreValue=s.ignoreValue)
    assert filled.groupSize[filled.recode[s.hole]] > 1 and filled.links > m.links
    # without the mark the hole's own values are one step from its neighbour's: within maxDistance
    unmarked = sc.reference_similar(s.table, s.columns, maxDistance=s.maxDistance)
    assert unmarked.groupSize[unmarked.recode[s.hole]] > 1
    assert m.maxSegId > S - 5200 and (m.groupSize[m.recode[s.high]] > 1).sum() > 20
    print('sparse_wide: %d entries, %d groups, %d links, %d records' % (len(s.table[1]), m.maxSegId, m.links, m.recordsSorted))


def test_large_raster_needs_a_second_trip():
    (rows, cols) = tc.RECODE_SHAPE
    assert rows * cols == 2201100 > tc.RECODE_ONE_TRIP == 2097152
    # the last workgroup of the second trip is partly beyond the groups of four labels
    assert (rows * cols // 4 - tc.RECODE_ONE_TRIP // 4) % 256 != 0
    block = tc.RECODE_BLOCK_ROWS * cols
    assert tc.RECODE_ONE_TRIP < block < rows * cols and (block // 4 - tc.RECODE_ONE_TRIP // 4) % 256 != 0
    assert 0 < rows - tc.RECODE_BLOCK_ROWS < tc.RECODE_BLOCK_ROWS
