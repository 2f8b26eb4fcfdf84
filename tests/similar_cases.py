"""The definition of neighbours.mergeSimilarSegments in numpy, and the cases the tests put through it.

The link rule is a boolean per entry of the table, written from the definition: d2(a, b) starts at +0.0 and adds, for
the columns in list order, t * t with t = x[a] - x[b] (numpy rounds every elementwise operation to float64 once, as
the library built without contraction does); an id with an ignored value (NaN, ignoreValue) in any column links to
nobody; an entry is a candidate when w >= minBorder, both ids are vertices, neither has an ignored value, d2 is finite
and -- with keys -- key[a] == key[b] != ignoreKey.  Without mutualNearest a candidate is a link when d2 <= thr2; with
it, when best[a] == b and best[b] == a (best: the candidate neighbour with the smallest d2, ties to the smallest id)
and d2 <= thr2.

Everything after the links goes through merge_cases: its components, its graph route to the contracted table and
its raster route."""
import numpy as np

import merge_cases as mc
import neighbour_cases as nc

MRG_PIECE = 2048            # entries per workgroup of the hook (csrc/nbrmerge.h)


def entries(table):
    """(a, b, w) of every entry: the row, the neighbour, the border length"""
    (offsets, nbrs, lens) = table
    a = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))
    return (a, nbrs.astype(np.int64), lens)


def widen(columns):
    return [np.asarray(col).astype(np.float64) for col in columns]


def ignored_ids(columns, ignoreValue=None):
    bad = np.zeros(len(columns[0]), dtype=bool)
    for x in widen(columns):
        bad |= np.isnan(x)
        if ignoreValue is not None:
            bad |= x == ignoreValue
    return bad


def distance2(columns, a, b):
    s = np.zeros(len(a), dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for x in widen(columns):
            t = x[a] - x[b]
            s = s + t * t
    return s


def link_model(table, columns, maxDistance=None, mutualNearest=False, ignoreValue=None, keys=None, ignoreKey=None,
               minBorder=1, segSize=None):
    """a Model with, per entry: candidate, d2, link; per id: best (0: no candidate); and thr2"""
    (a, b, w) = entries(table)
    S = len(table[0]) - 2
    vertex = np.ones(S + 1, dtype=bool)
    vertex[0] = False
    if segSize is not None:
        vertex &= np.asarray(segSize) > 0
    bad = ignored_ids(columns, ignoreValue)
    d2 = distance2(columns, a, b)
    cand = (w >= minBorder) & vertex[a] & vertex[b] & ~bad[a] & ~bad[b] & np.isfinite(d2)
    if keys is not None:
        k = np.asarray(keys).astype(np.int64)
        cand &= k[a] == k[b]
        if ignoreKey is not None:
            cand &= k[a] != ignoreKey
    m = mc.Model()
    (m.candidate, m.d2) = (cand, d2)
    m.thr2 = None if maxDistance is None else np.float64(maxDistance) * np.float64(maxDistance)
    m.best = np.zeros(S + 1, dtype=np.int64)
    if mutualNearest:
        idx = np.flatnonzero(cand)
        order = idx[np.lexsort((b[idx], d2[idx], a[idx]))]         # by row, then d2, then id
        first = np.ones(len(order), dtype=bool)
        first[1:] = a[order][1:] != a[order][:-1]
        m.best[a[order][first]] = b[order][first]
        link = cand & (m.best[a] == b) & (m.best[b] == a)
    else:
        assert maxDistance is not None
        link = cand.copy()
    if m.thr2 is not None:
        link &= d2 <= m.thr2
    m.link = link
    return m


def groups_from_links(table, link, segSize=None):
    """everything mergeSegments returns, from a boolean per entry: merge_cases' components and graph route (the part of
    merge_cases.reference_merge that follows its link rule)"""
    (a, b, lens) = entries(table)
    S = len(table[0]) - 2
    vertex = np.ones(S + 1, dtype=bool)
    vertex[0] = False
    if segSize is not None:
        vertex &= np.asarray(segSize) > 0
    m = mc.Model()
    m.links = int((link & (a < b)).sum())
    lab = mc.components(S + 1, a[link], b[link])
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
    m.table = mc.table_from_entries(ra[keep], rb[keep], lens[keep], m.maxSegId)
    return m


def ties_per_row(table, rule_model):
    """per id, the candidates of its row at the row's smallest d2 (2 or more: best was decided by the ids)"""
    (a, b, w) = entries(table)
    (cand, d2) = (rule_model.candidate, rule_model.d2)
    dmin = np.full(len(table[0]) - 1, np.inf)
    np.minimum.at(dmin, a[cand], d2[cand])
    return np.bincount(a[cand & (d2 == dmin[a])], minlength=len(dmin))


def reference_similar(table, columns, segSize=None, **rule):
    """the groups of the definition; the link model is kept as ``.rule``"""
    rule_model = link_model(table, columns, segSize=segSize, **rule)
    m = groups_from_links(table, rule_model.link, segSize)
    m.rule = rule_model
    return m


def same_as_key_merge():
    """groups_from_links restates the tail of merge_cases.reference_merge: with the key rule's links it must give
    what reference_merge gives (checked by the host tests on a real table)"""
    seg = nc.random_labels((65, 129), 40, 11)
    S = int(seg.max())
    table = nc.reference_neighbours(seg, True, S)
    keys = np.random.default_rng(1).integers(0, 4, size=S + 1)
    size = np.bincount(seg.ravel(), minlength=S + 1)
    (a, b, w) = entries(table)
    link = (keys[a] == keys[b]) & (size[a] > 0) & (size[b] > 0) & (a != 0) & (b != 0)
    return (groups_from_links(table, link, size), mc.reference_merge(table, keys, segSize=size))


# ---- columns -------------------------------------------------------------------------------------------------------
def integer_columns(S, C, seed, top=20, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, top + 1, size=S + 1).astype(dtype) for _ in range(C)]


def quarter_to_three_quarters(table, columns, **rule):
    """the smallest whole maxDistance at which at least a quarter of the candidates link, and that fraction"""
    m = link_model(table, columns, maxDistance=0, **rule)
    (a, b, w) = entries(table)
    d2 = m.d2[m.candidate & (a < b)]
    assert len(d2) > 20
    for dist in range(0, 1000):
        frac = float((d2 <= dist * dist).mean())
        if frac >= 0.25:
            return (dist, frac)
    raise AssertionError('no threshold below 1000')


def position_column(order):
    """col[label] = the label's position in the line ``order``: it rises by 1 per segment along the line"""
    col = np.zeros(len(order) + 1, dtype=np.float64)
    col[np.asarray(order)] = np.arange(len(order), dtype=np.float64)
    return col


def star_column(S, hub, near, nearValue=5.0):
    """the hub at 0, every other id far away and distinct (1000 + id), the ids ``near`` at ``nearValue``"""
    col = 1000.0 + np.arange(S + 1, dtype=np.float64)
    col[hub] = 0.0
    col[list(near)] = nearValue
    return col
