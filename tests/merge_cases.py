"""The definition of neighbours.mergeSegments in numpy, and the cases the tests put through it.

Entry (a, b, w) of a neighbour table is a link when key[a] == key[b], key[a] != ignoreKey and w >= minBorder (with
segSize: both ids have pixels).  A group is a connected component of the links over the ids 1..S; groups are numbered
1..M in ascending order of their smallest member; with segSize an id of size 0 belongs to no group and recodes to 0.
The contracted table adds w of every entry between two different groups to the groups' pair.

Two routes to the contracted table that share nothing: the graph route (the entries recoded and summed) and, where the
table came from a raster, the raster route (the neighbour table of the recoded raster, neighbour_cases)."""
import os

import numpy as np

import neighbour_cases as nc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


class Model(object):
    pass


def components(nrows, a, b):
    """lab[i] = the smallest id joined to i by the links (a[k], b[k]): minimum-label propagation to a fixpoint"""
    lab = np.arange(nrows, dtype=np.int64)
    while True:
        new = lab.copy()
        np.minimum.at(new, a, lab[b])
        np.minimum.at(new, b, lab[a])
        new = new[new]                      # (a label is a member of its own component: its label is a smaller one)
        if np.array_equal(new, lab):
            return lab
        lab = new


def table_from_entries(ra, rb, w, M):
    """CSR over 0..M of the entries (ra, rb, w), equal pairs summed"""
    key = (ra.astype(np.uint64) << np.uint64(32)) | rb.astype(np.uint64)
    (u, inv) = np.unique(key, return_inverse=True)
    total = np.zeros(len(u), dtype=np.int64)
    np.add.at(total, inv.reshape(-1), w.astype(np.int64))
    offsets = np.zeros(M + 2, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount((u >> np.uint64(32)).astype(np.int64), minlength=M + 1))
    return (offsets, (u & np.uint64(0xFFFFFFFF)).astype(np.uint32), total)


def reference_merge(table, keys, ignoreKey=None, minBorder=1, segSize=None):
    """The definition, from the table's three arrays (offsets, neighbours, borderLengths): a Model with recode,
    maxSegId, representative, groupSize, hist (None without segSize), links, recordsSorted and table, the contracted
    table by the graph route"""
    (offsets, nbrs, lens) = table
    S = len(offsets) - 2
    keys = np.asarray(keys).astype(np.int64)
    assert keys.shape == (S + 1,)
    a = np.repeat(np.arange(S + 1, dtype=np.int64), np.diff(offsets))
    b = nbrs.astype(np.int64)
    vertex = np.ones(S + 1, dtype=bool)
    vertex[0] = False
    if segSize is not None:
        vertex &= np.asarray(segSize) > 0
    link = (keys[a] == keys[b]) & (lens >= minBorder) & vertex[a] & vertex[b]
    if ignoreKey is not None:
        link &= keys[a] != ignoreKey
    m = Model()
    m.links = int((link & (a < b)).sum())
    lab = components(S + 1, a[link], b[link])
    roots = np.flatnonzero(vertex & (lab == np.arange(S + 1)))
    m.maxSegId = len(roots)
    number = np.zeros(S + 1, dtype=np.int64)
    number[roots] = np.arange(1, len(roots) + 1)
    m.recode = np.where(vertex, number[lab], 0).astype(np.uint32)
    m.representative = np.concatenate([[0], roots]).astype(np.uint32)
    m.groupSize = np.bincount(m.recode[vertex], minlength=m.maxSegId + 1).astype(np.int64)
    m.hist = None
    if segSize is not None:
        m.hist = np.zeros(m.maxSegId + 1, dtype=np.int64)
        np.add.at(m.hist, m.recode, np.asarray(segSize).astype(np.int64))
    (ra, rb) = (m.recode[a], m.recode[b])
    keep = (ra != rb) & (ra != 0) & (rb != 0)
    m.recordsSorted = int((keep & (a < b)).sum())
    m.table = table_from_entries(ra[keep], rb[keep], lens[keep], m.maxSegId)
    return m


def raster_route(seg, fourConnected, model):
    """the contracted table as the neighbour table of the recoded raster"""
    return nc.reference_neighbours(model.recode[seg], fourConnected, model.maxSegId)


# ---- the answers for neighbour_cases.EXAMPLE, by hand ----------------------------------------------------------
# [[1, 1, 2], [1, 3, 2], [0, 3, 3]]: 1-2, 1-3 and 2-3 all touch (four-connected borders 1, 2, 2).
# keys (0, 7, 7, 8): 1 and 2 merge, 3 stays.  New 1 = {1, 2}, new 2 = {3}; their border is 1-3 plus 2-3.
EXAMPLE_KEYS_A = np.array([0, 7, 7, 8], dtype=np.int32)
EXAMPLE_ANSWER_A = {
    'recode': [0, 1, 1, 2], 'maxSegId': 2, 'representative': [0, 1, 3], 'groupSize': [0, 2, 1], 'links': 1,
    'recordsSorted': 2, 'offsets': [0, 0, 1, 2], 'neighbours': [2, 1], 'lengths': {True: [4, 4], False: [8, 8]},
    'hist': [1, 5, 3]}
# keys (9, 4, 5, 4): 1 and 3 merge, 2 stays.  New 1 = {1, 3}, new 2 = {2}; their border is 1-2 plus 2-3.
EXAMPLE_KEYS_B = np.array([9, 4, 5, 4], dtype=np.uint8)
EXAMPLE_ANSWER_B = {
    'recode': [0, 1, 2, 1], 'maxSegId': 2, 'representative': [0, 1, 2], 'groupSize': [0, 2, 1], 'links': 1,
    'recordsSorted': 2, 'offsets': [0, 0, 1, 2], 'neighbours': [2, 1], 'lengths': {True: [3, 3], False: [6, 6]},
    'hist': [1, 6, 2]}


# ---- the cases ---------------------------------------------------------------------------------------------------
def line_raster(order, vertical):
    """a one-pixel-wide raster of the labels ``order``"""
    seg = np.asarray(order, dtype=np.uint32)
    return np.ascontiguousarray(seg.reshape(-1, 1) if vertical else seg.reshape(1, -1))


LINE = 4097


def line_descending():
    return np.arange(LINE, 0, -1)


def line_permuted():
    return np.random.default_rng(4097).permutation(np.arange(1, LINE + 1))


def through_a_third():
    """1 and 2 share two pixel pairs (four with the diagonals), each shares at least ten with 3"""
    seg = np.full((12, 20), 3, dtype=np.uint32)
    seg[0:2, 0:10] = 1
    seg[0:2, 10:20] = 2
    return seg


THROUGH_MIN_BORDER = 5


def mosaic():
    with np.load(os.path.join(GOLDEN, 'ci_scenario_1000.npz')) as z:
        return np.ascontiguousarray(z['mosaic'])


def _equal(S, seg):
    return np.zeros(S + 1, dtype=np.int64)


def _distinct(S, seg):
    return np.arange(S + 1, dtype=np.int64)


def _drawn(seed):
    def keys(S, seg):
        return np.random.default_rng(seed).integers(0, 4, size=S + 1).astype(np.int16)
    return keys


def _star_alternating(S, seg):
    """the hub's key is 0 (the hub is the label with the most pixels), the other ids alternate between 0 and 1"""
    keys = (np.arange(S + 1) % 2).astype(np.int64)
    keys[np.argmax(np.bincount(seg.ravel(), minlength=S + 1))] = 0
    return keys


def _mod5(S, seg):
    return (np.arange(S + 1) % 5).astype(np.uint32)


def _two_and_one(S, seg):
    return np.array([0, 1, 1, 2], dtype=np.int64)


class Case(object):
    """name; seg(): the raster; keys(S, seg): the key column; maxSegId: the table's last row (None: the largest
    label); ignoreKey, minBorder; sized: segSize is the raster's histogram"""
    def __init__(self, name, seg, keys, maxSegId=None, ignoreKey=None, minBorder=1, sized=False):
        (self.name, self.seg, self.keys, self.maxSegId) = (name, seg, keys, maxSegId)
        (self.ignoreKey, self.minBorder, self.sized) = (ignoreKey, minBorder, sized)

    def __repr__(self):
        return self.name


CASES = [
    Case('example_a', lambda: nc.EXAMPLE, lambda S, seg: EXAMPLE_KEYS_A),
    Case('example_b', lambda: nc.EXAMPLE, lambda S, seg: EXAMPLE_KEYS_B, sized=True),
    # nothing to merge: no segment at all, and one segment without a neighbour
    Case('no_segments', lambda: np.zeros((5, 7), dtype=np.uint32), _equal),
    Case('one_segment', lambda: np.ones((9, 70), dtype=np.uint32), _equal, sized=True),
    # all keys equal
    Case('equal_every_pixel', nc.every_pixel_its_own, _equal),
    Case('equal_enclosed', nc.enclosed_by_zeros, _equal),
    Case('equal_half_planes', nc.half_planes, _equal),
    # all keys distinct
    Case('distinct_random', lambda: nc.random_labels((65, 129), 40, 3), _distinct),
    Case('distinct_sparse_sized', nc.sparse_ids, _distinct, maxSegId=nc.SPARSE_MAX, sized=True),
    Case('distinct_sparse', nc.sparse_ids, _distinct, maxSegId=nc.SPARSE_MAX),
    # long find paths, hooks under later roots
    Case('row_descending', lambda: line_raster(line_descending(), False), _equal),
    Case('column_descending', lambda: line_raster(line_descending(), True), _equal),
    Case('row_permuted', lambda: line_raster(line_permuted(), False), _equal),
    Case('column_permuted', lambda: line_raster(line_permuted(), True), _equal),
    # the star
    Case('star', nc.hot_segment, _equal),
    Case('star_top', nc.hot_segment_top, _equal),
    Case('star_alternating', nc.hot_segment, _star_alternating),
    Case('star_top_alternating', nc.hot_segment_top, _star_alternating),
    # many groups whose smallest ids interleave
    Case('drawn_tiny', lambda: nc.random_labels((33, 65), 40, 10), _drawn(3)),
    Case('drawn_small', lambda: nc.random_labels((65, 129), 40, 11), _drawn(1)),
    Case('drawn_small_ignore', lambda: nc.random_labels((65, 129), 40, 11), _drawn(1), ignoreKey=2),
    Case('drawn_large', lambda: nc.random_labels((257, 300), 3000, 12), _drawn(2)),
    Case('drawn_large_ignore', lambda: nc.random_labels((257, 300), 3000, 12), _drawn(2), ignoreKey=2),
    # minBorder
    Case('half_planes_300', nc.half_planes, _equal, minBorder=300),
    Case('half_planes_301', nc.half_planes, _equal, minBorder=301),
    Case('through_a_third', through_a_third, _equal, minBorder=THROUGH_MIN_BORDER),
    Case('not_through_a_third', through_a_third, _two_and_one, minBorder=THROUGH_MIN_BORDER),
    # ids past 2^24 in the contraction's sort
    Case('wide_ids', nc.wide_ids, _equal, maxSegId=nc.WIDE_MAX),
    Case('wide_ids_distinct', nc.wide_ids, _distinct, maxSegId=nc.WIDE_MAX, sized=True),
    # a real table
    Case('mosaic', mosaic, _mod5, sized=True),
]
# what the border of the half planes is, so that 300 merges and 301 does not (four-connected; 898 with the diagonals)
HALF_PLANES_BORDER = {True: 300, False: 898}


def build(case, fourConnected):
    """(seg, S, keys, segSize or None, the table of seg by neighbour_cases) of a case"""
    seg = case.seg()
    S = case.maxSegId if case.maxSegId is not None else int(seg.max())
    table = nc.reference_neighbours(seg, fourConnected, S)
    size = np.bincount(seg.ravel(), minlength=S + 1).astype(np.int64) if case.sized else None
    return (seg, S, case.keys(S, seg), size, table)
