"""Neighbour tables built by hand for the merge chain (helpers of tests/test_table_cases_host.py,
tests/test_gpu_merge_tables.py and tests/test_gpu_merge_tables_dist.py; no tests here).

A table of test size that comes from a label raster is planar, has short border lengths and falls into the hook's
pieces of MRG_PIECE entries where it falls.  The library also takes a SegmentNeighbours or SegmentNeighboursShare put
together by hand, which may be any graph with any lengths: the generators below build the tables no raster gives.
A table is the tuple (offsets, neighbours, borderLengths) the models take (merge_cases.reference_merge,
similar_cases.reference_similar, merge_dist_cases.model); nothing here models the merge."""
import numpy as np

import merge_dist_cases as MD
import similar_cases as sc

PIECE = sc.MRG_PIECE
TWO32 = 1 << 32


def table_from_edges(S, a, b, w):
    """the symmetric CSR over the ids 0..S of the distinct edges a[k] < b[k] with lengths w[k]: offsets (int64,
    S + 2), neighbours (uint32, ascending within a row), borderLengths (int64); every pair is named from both sides"""
    (a, b, w) = (np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(w, dtype=np.int64))
    assert a.shape == b.shape == w.shape and a.ndim == 1
    assert len(a) == 0 or (a.min() >= 1 and b.max() <= S and (a < b).all())
    assert len(np.unique(a * (S + 1) + b)) == len(a), 'an edge is named twice'
    rows = np.concatenate([a, b])
    cols = np.concatenate([b, a])
    order = np.lexsort((cols, rows))
    offsets = np.zeros(S + 2, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(rows, minlength=S + 1))
    return (offsets, cols[order].astype(np.uint32), np.concatenate([w, w])[order])


def edges_of(table):
    """(a, b, w, e) of the entries a < b of a table, e their positions in the arrays"""
    (a, b, w) = sc.entries(table)
    e = np.flatnonzero(a < b)
    return (a[e], b[e], w[e], e)


def with_lengths(table, pairs, value):
    """a copy of the table with the length of the pairs (a, b) replaced from both sides"""
    (offsets, nbrs, lens) = table
    lens = lens.copy()
    for (a, b) in pairs:
        for (r, n) in ((a, b), (b, a)):
            (x, y) = (int(offsets[r]), int(offsets[r + 1]))
            lens[x + int(np.searchsorted(nbrs[x:y], n))] = value
    return (offsets, nbrs, lens)


def columns_of(table):
    """{'numNeighbours', 'borderLength'} of all ids, in numpy"""
    (a, _b, w) = sc.entries(table)
    total = np.zeros(len(table[0]) - 1, dtype=np.int64)
    np.add.at(total, a, w)
    return {'numNeighbours': np.diff(table[0]).astype(np.int64), 'borderLength': total}


def share_of(table, rank, world):
    """the SegmentNeighboursShare of distributed.idRange(rank, world, S): the rows as merge_dist_cases.share_rows cuts
    them, the columns of all ids"""
    from pyshepseg_amd import distributed, neighbours
    S = len(table[0]) - 2
    (lo, hi) = distributed.idRange(rank, world, S)
    (offsets, nbrs, lens) = MD.share_rows(table, lo, hi)
    return neighbours.SegmentNeighboursShare((lo, hi), S, True, np.ascontiguousarray(offsets), nbrs.copy(), lens.copy(),
                                             columns_of(table))


def whole_of(table):
    """the table as a SegmentNeighbours built by hand (copies: the table itself is left unchanged)"""
    from pyshepseg_amd import neighbours
    return neighbours.SegmentNeighbours(*[x.copy() for x in table], len(table[0]) - 2, True)


# ---- border lengths whose sums pass 2^32 ------------------------------------------------------------------------
GROUPS = 12
MEMBERS = 1100
MULT = [1, 2, 3, 63, 64, 65, 127, 129, 255, 256, 257, 1000]
WIDE_S = GROUPS * MEMBERS


def _member(g, k):
    """member k of group g: the groups' ids interleave, group g holds g + 1, g + 13, g + 25, ..."""
    return 1 + g + GROUPS * np.asarray(k, dtype=np.int64)


def _wide_edges(between, inside):
    """the chains inside the 12 groups (inside(g, k): the length between members k and k + 1) and, between group g and
    group (g + 1) % 12, MULT[g] edges between members of equal rank, taken from the low ranks where g is even and from
    the high ranks where it is odd (between(g, j): the length of the pair's j-th edge)"""
    (a, b, w) = ([], [], [])
    k = np.arange(MEMBERS - 1)
    for g in range(GROUPS):
        a.append(_member(g, k))
        b.append(_member(g, k + 1))
        w.append(inside(g, k))
        j = np.arange(MULT[g])
        rank = j if g % 2 == 0 else MEMBERS - 1 - j
        (x, y) = (_member(g, rank), _member((g + 1) % GROUPS, rank))
        a.append(np.minimum(x, y))
        b.append(np.maximum(x, y))
        w.append(between(g, j))
    return tuple(np.concatenate(v) for v in (a, b, w))


def wide_keys():
    """the key of an id is its group"""
    keys = np.zeros(WIDE_S + 1, dtype=np.int64)
    keys[1:] = np.arange(WIDE_S) % GROUPS
    return keys


def wide_sums():
    """(table, keys): 12 groups of 1100 ids chained by entries of length 1; the lengths between two groups cycle
    through 2^32 - 1, 2^31 and a drawn value, so the contraction's sums of 1 .. 1000 32-bit lengths pass 2^32"""
    rng = np.random.default_rng(232)

    def between(g, j):
        drawn = rng.integers(1, TWO32, size=len(j), dtype=np.int64)
        return np.where(j % 3 == 0, TWO32 - 1, np.where(j % 3 == 1, 1 << 31, drawn))
    (a, b, w) = _wide_edges(between, lambda g, k: np.ones(len(k), dtype=np.int64))
    return (table_from_edges(WIDE_S, a, b, w), wide_keys())


REFUSED = {'2^32': TWO32, '2^40': 1 << 40, '0': 0, '-5': -5}


def _first_middle_last(table, between):
    """three pairs (a, b) of the table's entries a < b that lie between two groups (``between``) or inside one: the
    first and the last of them in the arrays (they lie in the first and in the last piece) and the middle one"""
    keys = wide_keys()
    (a, b, _w, e) = edges_of(table)
    pick = np.flatnonzero((keys[a] != keys[b]) == between)
    pick = pick[[0, len(pick) // 2, -1]]
    return ([(int(a[i]), int(b[i])) for i in pick], e[pick])


def wide_refused(kind, between=True):
    """(table, keys, the positions of the three replaced entries a < b): wide_sums() with three lengths replaced by
    REFUSED[kind], between two groups (or, between=False, inside a group)"""
    (table, keys) = wide_sums()
    (pairs, at) = _first_middle_last(table, between)
    return (with_lengths(table, pairs, REFUSED[kind]), keys, at)


INSIDE_40 = 1 << 40
INSIDE_62 = 1 << 62


def wide_inside_groups():
    """(table, keys): lengths of 2^62 and 2^40 on entries inside a group only (the chain's steps 0, 4, 8, .. and 2, 6,
    10, .., a row holds one 2^62 at the most), 1 on the others; short lengths between the groups"""
    rng = np.random.default_rng(240)

    def inside(g, k):
        return np.where(k % 4 == 0, INSIDE_62, np.where(k % 4 == 2, INSIDE_40, 1))
    (a, b, w) = _wide_edges(lambda g, j: rng.integers(1, 1001, size=len(j), dtype=np.int64), inside)
    return (table_from_edges(WIDE_S, a, b, w), wide_keys())


# ---- rows at the edges of the hook's pieces -------------------------------------------------------------------------
FRONT = 3001            # empty rows in front of the first hub
GAP = 3050              # empty rows where a piece ends between two rows
BEHIND = 40             # empty rows behind the last leaf
NENTS = [PIECE * k + d for k in (1, 2, 3) for d in (-1, 0, 1)]
# nent -> (the hubs' degrees, the parity of the leaves whose key is the hubs')
GEOMETRY = {
    2047: ([1000, 23], 0), 2048: ([1024], 0), 2049: ([1024], 1),
    4095: ([2047], 0), 4096: ([2048], 0), 4097: ([2048], 1),
    6143: ([2047, 1024], 0), 6144: ([2047, 1025], 1), 6145: ([2048, 1024], 0)}


class Geometry(object):
    """table; keys (hubs 0, leaf j: (j + flip) % 2); column (the mutual rule's); segSize; hubs, leaves (ids); dangling:
    None or (a, b), the one entry named from one side only"""
    pass


def piece_geometry(nent):
    """A Geometry of exactly ``nent`` entries.  FRONT empty rows, then the hub rows (low ids) of the degrees of
    GEOMETRY over leaves (high ids) of one entry each: L leaves give the hub rows the entries 0 .. L - 1 and the leaf
    rows the entries L .. 2 L - 1.  GAP empty rows lie between the hubs and the leaves and in front of every leaf
    whose entry starts a piece, BEHIND empty rows behind the last leaf.

    A table that names every pair from both sides has an even number of entries.  An odd ``nent`` is the table of
    ``nent - 1`` with one more entry in the last leaf's row, which names an id b behind it that has no pixels
    (segSize[b] == 0) and no row: it is the last entry of the arrays, a < b, and by the definition no link, no
    candidate and no record.  Every other id has segSize 1.

    column: the hubs at 0, every leaf far away and distinct, but the leaf of a hub's last entry at 5 and -- flip 1 --
    the leaf of its first entry too: the hub's best is then decided between its first and its last entry."""
    (degrees, flip) = GEOMETRY[nent]
    L = sum(degrees)
    assert 2 * L + nent % 2 == nent
    g = Geometry()
    g.hubs = FRONT + 1 + np.arange(len(degrees), dtype=np.int64)
    ids = []
    at = int(g.hubs[-1]) + 1 + GAP
    for j in range(L):
        if j > 0 and (L + j) % PIECE == 0:
            at += GAP
        ids.append(at)
        at += 1
    g.leaves = np.array(ids, dtype=np.int64)
    S = at - 1 + BEHIND
    hubOf = np.repeat(g.hubs, degrees)
    table = table_from_edges(S, hubOf, g.leaves, 1 + np.arange(L) % 7)
    g.segSize = np.ones(S + 1, dtype=np.int64)
    g.dangling = None
    if nent % 2:
        (offsets, nbrs, lens) = table
        (a, b) = (int(g.leaves[-1]), S - 3)
        assert offsets[a + 1] == len(nbrs) and b > a
        offsets = offsets.copy()
        offsets[a + 1:] += 1
        table = (offsets, np.append(nbrs, np.uint32(b)), np.append(lens, np.int64(9)))
        g.segSize[b] = 0
        g.dangling = (a, b)
    g.table = table
    g.keys = np.full(S + 1, 7, dtype=np.int64)
    g.keys[g.hubs] = 0
    g.keys[g.leaves] = (np.arange(L) + flip) % 2
    first = g.leaves[np.cumsum(degrees) - np.asarray(degrees)]
    last = g.leaves[np.cumsum(degrees) - 1]
    g.column = sc.star_column(S, g.hubs, np.concatenate([first, last]) if flip else last)
    (g.first, g.last, g.flip) = (first, last, flip)
    return g


# ---- graphs that are not planar ---------------------------------------------------------------------------------
def random_graph(S=20000, degree=8, seed=5):
    """every id draws ``degree`` partners; the pairs deduplicated, lengths 1 .. 1000"""
    rng = np.random.default_rng(seed)
    x = np.repeat(np.arange(1, S + 1, dtype=np.int64), degree)
    y = rng.integers(1, S + 1, size=len(x), dtype=np.int64)
    keep = x != y
    (lo, hi) = (np.minimum(x, y)[keep], np.maximum(x, y)[keep])
    u = np.unique(lo * (S + 1) + hi)
    return table_from_edges(S, u // (S + 1), u % (S + 1), rng.integers(1, 1001, size=len(u), dtype=np.int64))


def class_keys(S, classes, seed=6):
    return np.random.default_rng(seed).integers(0, classes, size=S + 1).astype(np.int32)


def complete_bipartite(n=300):
    """(table, keys): every id of 1 .. n with every id of n + 1 .. 2 n, all keys equal: n * n links onto one root"""
    a = np.repeat(np.arange(1, n + 1, dtype=np.int64), n)
    b = np.tile(np.arange(n + 1, 2 * n + 1, dtype=np.int64), n)
    return (table_from_edges(2 * n, a, b, 1 + (a * 31 + b) % 97), np.zeros(2 * n + 1, dtype=np.int64))


def folded_chain(S=20000):
    """(table, keys): the edges (i, i + 1) and (i, S + 1 - i), all keys equal: every hook joins the two ends of what
    the chain has joined so far"""
    i = np.arange(1, S, dtype=np.int64)
    j = np.arange(1, (S + 1) // 2 + 1, dtype=np.int64)
    j = j[j < S + 1 - j]
    u = np.unique(np.concatenate([i * (S + 1) + i + 1, j * (S + 1) + S + 1 - j]))
    return (table_from_edges(S, u // (S + 1), u % (S + 1), 1 + u % 5), np.zeros(S + 1, dtype=np.int8))


# ---- ids past the first trip of the grid-stride loops -------------------------------------------------------------
SPARSE_S = 600000
ONE_TRIP = 2048 * 256           # ids a launch of 2048 workgroups reaches in one trip
SPARSE_IGNORE = 2               # one step from the columns' values: an id that is not marked as ignored would still link


class Sparse(object):
    """table; columns (float64, float32, int16), ignoreValue, maxDistance; high: the ids above ONE_TRIP with entries;
    hole: the one of them with an ignored value, holeFilled: the columns without it"""
    pass


def sparse_wide(S=SPARSE_S):
    """some 2000 pairs among the ids 1 .. 5000 and 300 among 200 ids above ONE_TRIP; every other id has no entries.
    The columns hold small integers, so about half of the pairs lie within maxDistance 1; one high id with a link
    has the ignore value in the last column."""
    rng = np.random.default_rng(600)
    s = Sparse()

    def pairs(pool, n):
        x = rng.choice(pool, size=n)
        y = rng.choice(pool, size=n)
        keep = x != y
        return np.unique(np.minimum(x, y)[keep] * (S + 1) + np.maximum(x, y)[keep])
    s.high = np.sort(rng.choice(np.arange(ONE_TRIP + 1, S + 1, dtype=np.int64), size=200, replace=False))
    u = np.concatenate([pairs(np.arange(1, 5001, dtype=np.int64), 2000), pairs(s.high, 300)])
    s.table = table_from_edges(S, u // (S + 1), u % (S + 1), rng.integers(1, 50, size=len(u), dtype=np.int64))
    cols = [rng.integers(0, 2, size=S + 1).astype(dt) for dt in (np.float64, np.float32, np.int16)]
    # the hole: a high id takes its first neighbour's values (a link), then the ignore value in the last column, where
    # the neighbour holds 1: d2 of the pair is 1, within maxDistance, so only the mark on the hole's record keeps them apart
    (offsets, nbrs, _lens) = s.table
    s.hole = int(s.high[np.flatnonzero(np.diff(offsets)[s.high] > 0)[-1]])
    near = int(nbrs[offsets[s.hole]])
    cols[2][near] = 1
    for col in cols:
        col[s.hole] = col[near]
    s.holeFilled = [col.copy() for col in cols]
    cols[2][s.hole] = SPARSE_IGNORE
    (s.columns, s.ignoreValue, s.maxDistance) = (cols, SPARSE_IGNORE, 1)
    return s


# ---- a raster of more labels than one trip of the recode ----------------------------------------------------------
RECODE_SHAPE = (1100, 2001)
RECODE_ONE_TRIP = 2048 * 256 * 4        # labels a launch of the recode reaches in one trip
RECODE_BLOCK_ROWS = 1050                # a block of 1050 rows is one trip and 3898 labels; the last block has 50 rows


def large_raster(S):
    """labels 0 .. S drawn for every pixel of RECODE_SHAPE"""
    return np.random.default_rng(2201).integers(0, S + 1, size=RECODE_SHAPE, dtype=np.uint32)
