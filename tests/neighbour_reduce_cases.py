"""The definition of neighbours.reduceOverNeighbours in numpy, and the tables the tests put through it.

Row r of the CSR table has entries with neighbour id n and border length w; v is the column as float64.  A value is
ignored when it is NaN or equals ignoreValue; C is the set of the row's entries whose v[n] is not ignored.  The
exact statistics (count, border, min, max, bordertohigher, nearest) are reduceat expressions; the three float sums
(mean, bordermean, meanabsdiff) are summed EXACTLY per row with math.fsum over error-free terms (a product w * y is
split into two exact products, a difference into its rounded value and its rounding error), then rounded once and
divided once: the model is within one unit in the last place of the true quotient, whatever the values."""
import math

import numpy as np

STATS = ('count', 'border', 'min', 'max', 'mean', 'bordermean', 'meanabsdiff', 'bordertohigher', 'nearest')
INT_STATS = ('count', 'border', 'bordertohigher', 'nearest')

# the thresholds of csrc/nbrreduce.h: rows above LONG entries leave the thread-per-row kernel, the LDS piece, the
# chunk of a long row
LONG = 256
PIECE = 1024
CHUNK = 4096
ROWS_PER_WORKGROUP = 256

ISSUE_DEGREES = [0, 1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]
THRESHOLD_DEGREES = [LONG - 1, LONG, LONG + 1, PIECE - 1, PIECE, PIECE + 1, CHUNK - 1, CHUNK, CHUNK + 1,
                     2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 63, 64, 65, 5, 0, 3]


def _split(y):
    """y = hi + lo exactly, both of at most 26 significant bits (Veltkamp)"""
    c = 134217729.0 * y
    hi = c - (c - y)
    return (hi, y - hi)


def _exact_products(w, y):
    """two arrays whose exact sum is w * y, for integers |w| < 2^26 held in float64"""
    (hi, lo) = _split(y)
    return (w * hi, w * lo)


def _two_diff(a, b):
    """(s, e): s = fl(a - b) and a - b = s + e exactly (Knuth)"""
    s = a - b
    bb = s - a
    e = (a - (s - bb)) - (b + bb)
    return (s, e)


def _row_fsum(parts, starts, n):
    """the correctly rounded sum of every row's terms; parts: arrays of terms in entry order, starts: n + 1 offsets
    (math.fsum per row, except where plain float64 sums are exact anyway)"""
    out = np.zeros(n, dtype=np.float64)
    rows = np.flatnonzero(np.diff(starts))
    stacked = np.stack(parts)
    if len(rows) and (stacked == np.rint(stacked)).all() and float(np.add.reduceat(np.abs(stacked).sum(axis=0),
                                                                                  starts[rows]).max()) < 2.0 ** 53:
        # integers whose absolute values sum below 2^53 in every row: every float64 summation order is exact
        out[rows] = np.add.reduceat(stacked.sum(axis=0), starts[rows])
        return out
    for r in np.flatnonzero(np.diff(starts)):
        out[r] = math.fsum(stacked[:, starts[r]:starts[r + 1]].ravel().tolist())
    return out


def reference_reduce(offsets, nbrs, lens, col, stats=STATS, ignoreValue=None, missing=-9999, withScales=False):
    """{statName: array of len(offsets) - 1 rows}.  withScales: also 'n' (counted entries) and, for the three float
    sums, 'scale:<statName>' = (sum w |x|) / sum w with x the summed term (w = 1 for mean): what the error bound of
    a float64 summation in any order is stated in."""
    offsets = np.asarray(offsets, dtype=np.int64)
    nbrs = np.asarray(nbrs).astype(np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    v = np.asarray(col).astype(np.float64)
    nrows = len(offsets) - 1
    assert len(v) == nrows and offsets[0] == 0 and offsets[-1] == len(nbrs) == len(lens)
    if lens.size and int(lens.max()) >= 1 << 26:
        # _exact_products wants |w| < 2^26.  Longer lengths are as exact where the column holds integers of at most 26
        # bits (y splits into y + 0) and no row's sum of w (1 + 2 max|v|) reaches 2^53: every product, difference and
        # partial sum is then an integer float64 holds
        known = v[~np.isnan(v)]
        top = float(np.abs(known).max()) if known.size else 0.0
        assert (known == np.rint(known)).all() and top < 1 << 26
        assert (lens >= 0).all() and float(np.add.reduceat(lens.astype(np.float64), offsets[:-1][np.diff(offsets) > 0]).max()) \
            * (1.0 + 2.0 * top) < 2.0 ** 53

    def ignored(x):
        bad = np.isnan(x)
        if ignoreValue is not None:
            bad |= x == ignoreValue
        return bad
    row = np.repeat(np.arange(nrows, dtype=np.int64), np.diff(offsets))
    keep = ~ignored(v[nbrs])
    (row, n, w) = (row[keep], nbrs[keep], lens[keep])
    x = v[n]
    count = np.bincount(row, minlength=nrows).astype(np.int64)
    starts = np.zeros(nrows + 1, dtype=np.int64)
    starts[1:] = np.cumsum(count)
    rows = np.flatnonzero(count)
    first = starts[rows]
    own_ok = ~ignored(v)
    have = count > 0
    own_have = have & own_ok
    wf = w.astype(np.float64)

    def fill_float(values, where):
        out = np.full(nrows, float(missing), dtype=np.float64)
        out[where] = values[where]
        return out

    def per_row(ufunc, values, dtype):
        out = np.zeros(nrows, dtype=dtype)
        if len(rows):
            out[rows] = ufunc.reduceat(values, first)
        return out
    border = per_row(np.add, w, np.int64)
    res = {'count': count, 'border': border}
    res['min'] = fill_float(per_row(np.minimum, x, np.float64), have)
    res['max'] = fill_float(per_row(np.maximum, x, np.float64), have)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        res['mean'] = fill_float(_row_fsum([x], starts, nrows) / count, have)
        bf = border.astype(np.float64)
        res['bordermean'] = fill_float(_row_fsum(_exact_products(wf, x), starts, nrows) / bf, have)
        # |x - own| = |s| + sign(s) e, with s the rounded difference and e its error (e = 0 where s = 0)
        own = v[row]
        (s, e) = _two_diff(x, own)
        sign = np.where(s < 0, -1.0, 1.0)
        terms = _exact_products(wf, np.abs(s)) + _exact_products(wf, sign * e)
        res['meanabsdiff'] = fill_float(_row_fsum(terms, starts, nrows) / bf, own_have)
        higher = per_row(np.add, np.where(x > own, w, 0), np.int64)
        res['bordertohigher'] = np.where(own_have, higher, 0).astype(np.int64)
        # the smallest distance of the row, then the smallest id that has it (the distance as float64 rounds it:
        # the comparison of two distances is the one the kernel makes)
        d = np.abs(x - own)
        dmin = per_row(np.minimum, d, np.float64)
        big = np.int64(1) << np.int64(40)
        cand = np.where(d == dmin[row], n, big)
        near = per_row(np.minimum, cand, np.int64)
        res['nearest'] = np.where(own_have & (near < big), near, 0).astype(np.int64)
        if withScales:
            res['n'] = count
            res['scale:mean'] = per_row(np.add, np.abs(x), np.float64) / np.maximum(count, 1)
            res['scale:bordermean'] = per_row(np.add, wf * np.abs(x), np.float64) / np.maximum(bf, 1)
            res['scale:meanabsdiff'] = per_row(np.add, wf * d, np.float64) / np.maximum(bf, 1)
    extra = [k for k in res if k not in STATS]
    return {k: res[k] for k in list(stats) + (extra if withScales else [])}


def table_with_degrees(degrees, seed, maxLength=1 << 17):
    """(offsets, nbrs, lens, maxSegId): row i + 1 has degrees[i] strictly ascending random ids, none its own; border
    lengths random in 1..maxLength.  The table need not be symmetric.  Rows are added behind the given ones (with
    no entries) until the largest degree is possible."""
    degrees = np.asarray(degrees, dtype=np.int64)
    rng = np.random.default_rng(seed)
    maxSegId = max(len(degrees), int(degrees.max()) + 1 if len(degrees) else 0)
    offsets = np.zeros(maxSegId + 2, dtype=np.int64)
    offsets[2:2 + len(degrees)] = np.cumsum(degrees)
    offsets[2 + len(degrees):] = offsets[1 + len(degrees)]
    nbrs = np.empty(int(degrees.sum()), dtype=np.uint32)
    big = np.flatnonzero(degrees > 64)
    for i in big:
        # ids 1..maxSegId without the row's own, a sorted sample
        pick = np.sort(rng.choice(maxSegId - 1, size=int(degrees[i]), replace=False)) + 1
        pick[pick >= i + 1] += 1
        nbrs[offsets[i + 1]:offsets[i + 2]] = pick
    small = np.flatnonzero((degrees > 0) & (degrees <= 64))
    if len(small):
        # many short rows at once: distinct ids by sorting random keys per row is too slow for 10^5 rows in a
        # loop, so draw with replacement, sort, and spread ties apart: ascending gaps of at least 1
        total = int(degrees[small].sum())
        rowOf = np.repeat(small, degrees[small])
        pos = np.arange(total) - np.repeat(np.cumsum(degrees[small]) - degrees[small], degrees[small])
        room = (maxSegId - 1) - degrees[rowOf]              # ids left over once every entry has one
        base = np.floor(rng.random(total) * (room + 1)).astype(np.int64)
        order = np.lexsort((base, rowOf))
        base = base[order]                                  # ascending within a row (rowOf is sorted already)
        pick = base + pos + 1                               # strictly ascending, in 1..maxSegId - 1
        pick[pick >= rowOf + 1] += 1
        dest = np.repeat(offsets[small + 1], degrees[small]) + pos
        nbrs[dest] = pick
    lens = rng.integers(1, maxLength + 1, size=len(nbrs), dtype=np.int64)
    return (offsets, nbrs, lens, maxSegId)


def table_violations(offsets, nbrs, lens):
    """the rules shp_nbr_upload checks, as a list of the names of those broken"""
    offsets = np.asarray(offsets, dtype=np.int64)
    nbrs = np.asarray(nbrs).astype(np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    bad = []
    if offsets[0] != 0 or offsets[1] != 0:
        bad.append('first')
    if (np.diff(offsets) < 0).any():
        bad.append('decreasing')
    if offsets[-1] != len(nbrs):
        bad.append('end')
    if bad:
        return bad
    maxSegId = len(offsets) - 2
    row = np.repeat(np.arange(maxSegId + 1, dtype=np.int64), np.diff(offsets))
    if ((nbrs < 1) | (nbrs > maxSegId)).any():
        bad.append('range')
    if (nbrs == row).any():
        bad.append('self')
    inner = np.ones(len(nbrs), dtype=bool)
    inner[offsets[:-1][np.diff(offsets) > 0]] = False       # a row's first entry has no predecessor
    if (inner[1:] & (nbrs[1:] <= nbrs[:-1])).any():
        bad.append('order')
    if (lens < 1).any():
        bad.append('length')
    return bad


SPAN_LONG_ROWS = (3000, 70000, 300000)


def span_degrees(seed=11):
    """100 000 rows of geometric degrees (mean 6) with rows of 3 000, 70 000 and 300 000 entries in the middle"""
    rng = np.random.default_rng(seed)
    deg = rng.geometric(1.0 / 7.0, size=100000).astype(np.int64) - 1        # mean 6, from 0
    deg[49999:50002] = SPAN_LONG_ROWS
    return deg


def span_table():
    """the span case: its rows straddle every piece and chunk edge; border lengths 1..2^10"""
    return table_with_degrees(span_degrees(), 12, maxLength=1 << 10)


def integer_column(nrows, bound, seed, dtype=np.float64):
    """integers in -bound..bound"""
    return np.random.default_rng(seed).integers(-bound, bound + 1, size=nrows).astype(dtype)


def real_column(nrows, seed):
    """float64 uniform in (-1000, 1000)"""
    return np.random.default_rng(seed).uniform(-1000.0, 1000.0, size=nrows)
