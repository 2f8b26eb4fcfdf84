"""The definition of neighbours.aggregateToGroups in numpy, and the raster whose merge gives groups of every size the
kernels' paths turn on.

Group g's members are the old ids i with recode[i] == g in ascending order; C is the set of members whose value is
not ignored (NaN, or equal to ignoreValue).  Two routes:
  exact route   numpy.bincount / ufunc.at expressions, for columns and weights whose every sum is exact in any order;
  order route   the float sums restated in the order csrc/nbrreduce.h gives a row of the group's length: a plain loop
                up to LONG members; above that chunks of CHUNK members by position, in a chunk the 64 strided lane
                sums and the butterfly acc = acc + acc[lane ^ d] for d = 32 .. 1, then the chunks in order.
and, for the bound on real-valued columns, the correctly rounded sums by math.fsum (neighbour_reduce_cases)."""
import numpy as np

import merge_cases as mc
import neighbour_cases as nc
import neighbour_reduce_cases as rc

STATS = ('count', 'weight', 'min', 'max', 'sum', 'mean', 'weightedmean')
INT_STATS = ('count', 'weight')

# members per group, in the order of the groups along the line; behind the group of 2 lies an id without pixels
RUN_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193]
LADDER = 300                # members of each of the two interleaved groups


def raster():
    """(seg, S, keys, emptyId, ladderBase).  Row 0: the ids 1 .. in a line, their keys in runs of RUN_SIZES (one id
    behind the run of 2 is left out of the raster: it has no pixels).  Row 1: zeros.  Rows 2 and 3: a ladder, the ids
    base, base + 2, .. above and base + 1, base + 3, .. below, with keys (id - base) % 2: two groups whose members
    interleave."""
    runs = sum(RUN_SIZES)
    emptyId = 1 + RUN_SIZES[0] + RUN_SIZES[1]
    base = runs + 2
    S = base + 2 * LADDER - 1
    seg = np.zeros((4, runs + 1), dtype=np.uint32)
    seg[0] = np.arange(1, runs + 2)
    seg[0, emptyId - 1] = 0
    seg[2, :LADDER] = base + 2 * np.arange(LADDER)
    seg[3, :LADDER] = base + 1 + 2 * np.arange(LADDER)
    keys = np.zeros(S + 1, dtype=np.int64)
    sizes = list(RUN_SIZES)
    sizes[2:2] = [1]                                            # (the id without pixels takes a key of its own)
    keys[1:base] = np.repeat(np.arange(len(sizes)), sizes)
    keys[base:] = 100 + (np.arange(2 * LADDER) % 2)
    return (seg, S, keys, emptyId, base)


def member_csr(recode, M):
    """(offsets over 0..M, members): the ids of every group, ascending"""
    recode = np.asarray(recode).astype(np.int64)
    order = np.argsort(recode, kind='stable')
    order = order[recode[order] != 0]
    offsets = np.zeros(M + 2, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(recode[order], minlength=M + 1))
    return (offsets, order.astype(np.uint32))


def ignored(x, ignoreValue):
    bad = np.isnan(x)
    if ignoreValue is not None:
        bad |= x == ignoreValue
    return bad


def ordered_sum(terms, keep):
    """the float64 sum of terms[keep] in the order of csrc/nbrreduce.h for a row of len(terms) entries"""
    n = len(terms)
    if n <= rc.LONG:
        acc = np.float64(0.0)
        for (t, k) in zip(terms, keep):
            if k:
                acc = acc + t
        return acc
    lane = np.arange(64)
    total = np.float64(0.0)
    for c0 in range(0, n, rc.CHUNK):
        chunk = np.where(keep[c0:c0 + rc.CHUNK], terms[c0:c0 + rc.CHUNK], 0.0)     # (x + 0.0 == x: no sum here is -0.0)
        padded = np.zeros(-(-len(chunk) // 64) * 64, dtype=np.float64)
        padded[:len(chunk)] = chunk
        acc = np.zeros(64, dtype=np.float64)
        for row in padded.reshape(-1, 64):
            acc = acc + row
        for d in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lane ^ d]
        total = total + acc[0]
    return total


def reference_aggregate(recode, M, col, weights=None, ignoreValue=None, missing=-9999, route='exact'):
    """{statName: M + 1 rows}; route 'exact', 'order' or 'fsum' (with 'n', 'scale:sum', 'scale:mean' and
    'scale:weightedmean' for the bound)"""
    recode = np.asarray(recode).astype(np.int64)
    raw = np.asarray(col)
    v = raw.astype(np.float64)
    w = np.ones(len(v), dtype=np.int64) if weights is None else np.asarray(weights).astype(np.int64)
    keep = ~ignored(v, ignoreValue) & (recode != 0)
    g = recode[keep]
    count = np.bincount(g, minlength=M + 1).astype(np.int64)
    weight = np.zeros(M + 1, dtype=np.int64)
    np.add.at(weight, g, w[keep])
    have = count > 0
    res = {'count': count, 'weight': weight}

    def fill(values, where):
        out = np.full(M + 1, float(missing), dtype=np.float64)
        out[where] = values[where]
        return out
    lo = np.full(M + 1, np.inf)
    np.minimum.at(lo, g, v[keep])
    hi = np.full(M + 1, -np.inf)
    np.maximum.at(hi, g, v[keep])
    res['min'] = fill(lo, have)
    res['max'] = fill(hi, have)
    wf = w.astype(np.float64)
    if route == 'exact':
        fsum = np.bincount(g, weights=v[keep], minlength=M + 1)
        wsum = np.bincount(g, weights=(wf * v)[keep], minlength=M + 1)
    else:
        (offsets, members) = member_csr(recode, M)
        m = members.astype(np.int64)
        if route == 'order':
            fsum = np.zeros(M + 1)
            wsum = np.zeros(M + 1)
            for grp in range(1, M + 1):
                ids = m[offsets[grp]:offsets[grp + 1]]
                fsum[grp] = ordered_sum(v[ids], keep[ids])
                wsum[grp] = ordered_sum(wf[ids] * v[ids], keep[ids])
        else:
            # the kept members only, in member order: the rows of neighbour_reduce_cases._row_fsum
            mk = m[keep[m]]
            starts = np.zeros(M + 2, dtype=np.int64)
            starts[1:] = np.cumsum(count)
            fsum = rc._row_fsum([v[mk]], starts, M + 1)
            wsum = rc._row_fsum(rc._exact_products(wf[mk], v[mk]), starts, M + 1)
            res['n'] = count
            res['scale:sum'] = np.bincount(g, weights=np.abs(v[keep]), minlength=M + 1)
            res['scale:mean'] = res['scale:sum'] / np.maximum(count, 1)
            res['scale:weightedmean'] = np.bincount(g, weights=(wf * np.abs(v))[keep], minlength=M + 1) / np.maximum(weight, 1)
    if raw.dtype.kind in 'iu':
        isum = np.zeros(M + 1, dtype=np.int64)
        np.add.at(isum, g, raw.astype(np.int64)[keep])
        res['sum'] = isum
    else:
        res['sum'] = fill(fsum, have)
    with np.errstate(invalid='ignore', divide='ignore'):
        res['mean'] = fill(fsum / count, have)
        res['weightedmean'] = fill(wsum / weight.astype(np.float64), have & (weight > 0))
    return res
