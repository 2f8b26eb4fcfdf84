"""The cases of tests/test_gpu_stats_edges.py -- csrc/segstats.h's three reducers (k_seg_stats: a thread per segment,
k_seg_stats_big: a wavefront per segment, k_stats_patch / k_stats_patch_bands: an LDS table and a rank sort per patch)
on rasters built to stand on either side of the constants that choose between them -- with what they are compared
against and what they reach.

Importable without a GPU: tests/test_stats_edge_cases_host.py runs the census of every case, the numpy model against
the oracle, and the high-precision bound on the oracle itself.  Every size below is derived from the constants parsed
out of segstats.h, so a change of a constant moves the cases with it.

Three references:
 * oracle.segstats, the project's restatement of the reference (pinned to the reference's goldens): every column of
   every entry must have its bits;
 * int_model: the integer statistics from a per-segment sorted value array, written independently in numpy;
 * float_violations: the float columns against exact arithmetic -- the mean must be float32(float(exact sum) / n),
   the stddev's square must lie within (D + 3) * 2^-24 (relative) of the variance around that float32 mean computed
   in rationals, D the segment's distinct values.  The variance is a sum of D non-negative float32 terms: one
   rounding per term (the float64 work before it is 2^-29 of that), at most D - 1 float32 additions whose partial
   sums never exceed the total, and the final float32 rounding of the square root, which is two roundings' worth on
   its square: D + 2, rounded up to D + 3.  This is the safety net; the assertion that matters is bit equality with
   the oracle.

The percentile scan (percentile_float_pairs): n * (p / 100.0) in floats lands just above an integer for 586 (n, p)
below n = 4200 -- (25, 28), (25, 56), (50, 14), (50, 28), (50, 56), (100, 7) among them -- and the reference's index
is the float one.  Case A8 holds a segment for every such n up to SPP_MAXRUN and a handful up to SEGSTATS_BIG, with the
percentile parameters of all of them as columns; the same
scan between SEGSTATS_BIG + 1 and 3 * SEGSTATS_BIG finds pairs too (test_stats_edge_cases_host.py counts them), and
the wavefront path gets three of them.
"""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pyshepseg_amd', 'csrc')


def _define(text, name):
    m = re.search(r'^#define\s+%s\s+(\d+)u?\b' % name, text, flags=re.M)
    assert m, 'no #define %s' % name
    return int(m.group(1))


def _constants():
    text = open(os.path.join(CSRC, 'segstats.h')).read()
    names = ('SEGSTATS_STAGE', 'SEGSTATS_BIG', 'SPP_MAXRUN', 'SPP_MAXDIST', 'SPP_SLOTS', 'SPP_H', 'SPP_W')
    out = [_define(text, n) for n in names]
    grid = re.search(r'hipLaunchKernelGGL\(k_seg_stats_big, dim3\((\d+)\), dim3\(256\)', text)
    assert grid, 'k_seg_stats_big is no longer launched as a fixed grid of 256-thread workgroups'
    hashes = set(re.findall(r'\* (\d+)u\) >> (\d+);', text))
    assert len(hashes) == 1, 'the patch kernels no longer share one hash'
    (mul, shift) = hashes.pop()
    return out + [int(grid.group(1)) * 4, int(mul), int(shift)]


STAGE, BIG, MAXRUN, MAXDIST, SLOTS, PH, PW, BIG_WAVES, HASH_MUL, HASH_SHIFT = _constants()
PATCH = PH * PW
M32 = 0xFFFFFFFF
PCS = (0, 1, 50, 99, 100)
BASE = (('mn', 'min'), ('mx', 'max'), ('mean', 'mean'), ('sd', 'stddev'), ('med', 'median'), ('mode', 'mode'),
        ('n', 'pixcount'))
LIMITS = {'uint8': (0, 255), 'int16': (-32768, 32767), 'uint16': (0, 65535), 'int32': (-2 ** 31, 2 ** 31 - 1),
          'uint32': (0, M32)}


def selection(pcs=PCS, prefix=''):
    """all eight statistics, the percentile once per parameter of pcs"""
    return [(prefix + a, b) for (a, b) in BASE] + [('%sp%d' % (prefix, p), 'percentile', p) for p in pcs]


def int_names(pcs=PCS):
    """the integer columns of selection(pcs), in the order the oracle and the library number them"""
    return [s[0] for s in selection(pcs) if s[1] not in ('mean', 'stddev')]


def home_slot(ids):
    """the kernels' hash: the slot a label probes first"""
    return ((np.asarray(ids, dtype=np.uint64) * np.uint64(HASH_MUL)) & np.uint64(M32)) >> np.uint64(HASH_SHIFT)


def ids_with_home(slot, count, start=1):
    """the first `count` ids from `start` on whose home slot is `slot`"""
    out = []
    lo = start
    while len(out) < count:
        ids = np.arange(lo, lo + 65536, dtype=np.uint64)
        out.extend(int(i) for i in ids[home_slot(ids) == slot])
        lo += 65536
    return out[:count]


def mix(i, salt=0):
    """a fixed 32-bit scramble of the integers i (content for bands: no random state to keep)"""
    x = (np.asarray(i, dtype=np.uint64) + np.uint64(salt * 7919 + 1)) * np.uint64(0x9E3779B1) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = x * np.uint64(0x85EBCA77) & np.uint64(M32)
    x ^= x >> np.uint64(13)
    return x


# ---- the percentile scan ---------------------------------------------------------------------------------------------
def percentile_index(n, p):
    """the reference's element: ceil(n * (p / 100)) - 1 in floats, the last one for p = 0"""
    t = n * (p / 100.0)
    return n - 1 if t <= 0.0 else min(int(math.ceil(t)), n) - 1


def percentile_float_pairs(n_lo, n_hi):
    """(n, p), n_lo <= n < n_hi, 0 <= p <= 100, whose float index differs from the exact ceil(n p / 100) - 1"""
    n = np.arange(n_lo, n_hi, dtype=np.int64)[:, None]
    p = np.arange(0, 101, dtype=np.int64)[None, :]
    flt = np.ceil(n.astype(np.float64) * (p.astype(np.float64) / 100.0)).astype(np.int64)
    exact = -((-n * p) // 100)
    (i, j) = np.nonzero(flt != exact)
    return [(int(n[a, 0]), int(p[0, b])) for (a, b) in zip(i, j)]


# ---- the references --------------------------------------------------------------------------------------------------
def _valid_sorted(seg, band, null, S):
    """(ids that have valid pixels, first index, count, values sorted by (id, value))"""
    s = np.asarray(seg).reshape(-1)
    v = np.asarray(band).reshape(-1).astype(np.int64)
    ok = (s != 0) & (s <= S)
    if null is not None:
        ok &= v != int(null)
    (s, v) = (s[ok], v[ok])
    order = np.lexsort((v, s))
    (s, v) = (s[order], v[order])
    (ids, first, cnt) = np.unique(s, return_index=True, return_counts=True)
    return ids, first, cnt, v


def int_model(seg, band, null, S, missing=-9999, pcs=PCS):
    """{column name: int64 column} of the integer statistics of selection(pcs)"""
    names = int_names(pcs)
    cols = {k: np.full(S + 1, missing, dtype=np.int64) for k in names}
    cols['n'][:] = 0
    for k in names:
        cols[k][0] = 0
    (ids, first, cnt, v) = _valid_sorted(seg, band, null, S)
    for (i, f, n) in zip(ids.tolist(), first.tolist(), cnt.tolist()):
        a = v[f:f + n]
        (u, c) = np.unique(a, return_counts=True)
        cols['n'][i] = n
        cols['mn'][i] = a[0]
        cols['mx'][i] = a[-1]
        cols['mode'][i] = u[np.argmax(c)]            # the first of the largest counts: the smallest such value
        cols['med'][i] = a[percentile_index(n, 50)]
        for p in pcs:
            cols['p%d' % p][i] = a[percentile_index(n, p)]
    return cols


def float_violations(seg, band, null, S, missing, mean_col, sd_col):
    """the rows whose mean is not float32(float(exact sum) / n) or whose stddev breaks the (D + 3) * 2^-24 bound, as
    text ('' when there are none); rows without valid pixels must hold float32(missing), row 0 zero"""
    bad = []
    (ids, first, cnt, v) = _valid_sorted(seg, band, null, S)
    empty = np.ones(S + 1, dtype=bool)
    empty[ids] = False
    empty[0] = False
    miss = np.float32(missing)
    if mean_col[0] != 0 or sd_col[0] != 0:
        bad.append('row 0 is not zero')
    if not ((mean_col[empty] == miss).all() and (sd_col[empty] == miss).all()):
        bad.append('a row without valid pixels is not float32(missing)')
    for (i, f, n) in zip(ids.tolist(), first.tolist(), cnt.tolist()):
        a = v[f:f + n]
        (u, c) = np.unique(a, return_counts=True)
        mean = np.float32(int(a.sum()) / n)
        if mean.view(np.uint32) != mean_col[i].view(np.uint32):
            bad.append('id %d: mean %r, exact %r' % (i, mean_col[i], mean))
            continue
        m = Fraction(float(mean))
        num = sum(ci * (ui * m.denominator - m.numerator) ** 2 for (ui, ci) in zip(u.tolist(), c.tolist()))
        var = Fraction(num, m.denominator ** 2 * n)
        sd = Fraction(float(sd_col[i]))
        if abs(sd * sd - var) > Fraction(len(u) + 3, 1 << 24) * var:
            bad.append('id %d: stddev %r, exact variance %r (D = %d)' % (i, sd_col[i], float(var), len(u)))
    return '; '.join(bad[:5])


# ---- what a case reaches ---------------------------------------------------------------------------------------------
def flat_keys(seg, band, null, S):
    """the segment key of every pixel as k_stats_keys makes it: nodata pixels, the null segment and ids above S are
    keyed to 0"""
    s = np.asarray(seg).reshape(-1).astype(np.int64)
    key = np.where(s > S, 0, s)
    if null is not None:
        key = np.where(np.asarray(band).reshape(-1).astype(np.int64) == int(null), 0, key)
    return key


def sort_census(keys, S):
    """the sort path over these pairs, per wavefront of 64 consecutive ids (id 0 included, with the pairs keyed to
    it): span (values its ids hold together), staged (through LDS or read from memory); cnt per id; big (ids that go to
    k_seg_stats_big -- id 0 never does)"""
    cnt = np.bincount(keys, minlength=S + 1).astype(np.int64)
    off = np.cumsum(cnt) - cnt
    first = np.arange(S // 64 + 1) * 64
    last = np.minimum(first + 63, S)
    span = off[last] + cnt[last] - off[first]
    big = np.flatnonzero(cnt > BIG)
    return {'cnt': cnt, 'span': span, 'staged': span <= STAGE, 'big': big[big != 0]}


def patch_census(seg, band, null, S):
    """per 32 x 64 patch, row-major: a dict of
    ndist (distinct labels), crowded, ids, pix / valid (per label, pixels here), complete1 / completeN (per label: the
    one-band rule -- valid pixels <= SPP_MAXRUN -- and the several-band rule -- all pixels), left1 / leftN (pixels
    that go to the sorts), words1 / wordsN (entries of runs[] taken: every run and one unused entry behind it),
    chain (the longest probe chain), wrapped (a label sits below its home slot), noslot_labels, noslot_pixels.
    Slots are given in raster order of a label's first pixel: the kernel's order is whatever the hardware makes it,
    but which SLOTS end up taken does not depend on the order, nor does how many labels find none.
    Also returns flagged1 / flaggedN: per id, whether its row is the sort path's."""
    seg = np.asarray(seg)
    (H, W) = seg.shape
    lab = (seg != 0) & (seg <= S)
    valid = lab.copy()
    if null is not None:
        valid &= np.asarray(band).astype(np.int64) != int(null)
    tot = np.bincount(seg[lab], minlength=S + 1)
    (flagged1, flaggedN) = (np.zeros(S + 1, dtype=bool), np.zeros(S + 1, dtype=bool))
    out = []
    for y0 in range(0, H, PH):
        for x0 in range(0, W, PW):
            m = lab[y0:y0 + PH, x0:x0 + PW].reshape(-1)
            labs = seg[y0:y0 + PH, x0:x0 + PW].reshape(-1)[m]
            vm = valid[y0:y0 + PH, x0:x0 + PW].reshape(-1)[m]
            (ids, firstpx, inv, pix) = np.unique(labs, return_index=True, return_inverse=True, return_counts=True)
            nvalid = np.bincount(inv[vm], minlength=len(ids))
            crowded = len(ids) > MAXDIST
            here = pix == tot[ids]
            c1 = here & (nvalid <= MAXRUN) & (not crowded)
            cN = here & (pix <= MAXRUN) & (not crowded)
            flagged1[ids[~c1]] = True
            flaggedN[ids[~cN]] = True
            taken = bytearray(SLOTS)
            (chain, wrapped, noslot) = (0, False, [])
            order = np.argsort(firstpx, kind='stable')
            homes = home_slot(ids[order]).tolist()
            for (k, home) in zip(order.tolist(), homes):
                (h, d) = (home, 0)
                while d < SLOTS and taken[h]:
                    (h, d) = ((h + 1) & (SLOTS - 1), d + 1)
                if d == SLOTS:
                    noslot.append(k)
                    continue
                taken[h] = 1
                chain = max(chain, d)
                wrapped = wrapped or h < home
            out.append({'ndist': len(ids), 'crowded': crowded, 'ids': ids, 'pix': pix, 'valid': nvalid,
                        'complete1': c1, 'completeN': cN, 'left1': int(nvalid[~c1].sum()), 'leftN': int(pix[~cN].sum()),
                        'words1': int((nvalid[c1] + 1).sum()), 'wordsN': int((pix[cN] + 1).sum()), 'chain': chain,
                        'wrapped': wrapped, 'noslot_labels': len(noslot), 'noslot_pixels': int(pix[noslot].sum())})
    return out, flagged1, flaggedN


def left_keys(seg, band, null, S, flagged, one_band):
    """the keys of the pairs the patch path hands to the sorts: the valid pixels of flagged labels (k_stats_patch),
    or all their pixels with the nodata ones keyed to 0 (k_stats_patch_bands + k_stats_left_keys)"""
    s = np.asarray(seg).reshape(-1).astype(np.int64)
    take = (s != 0) & (s <= S)
    take[take] = flagged[s[take]]
    key = flat_keys(seg, band, null, S)
    if one_band:
        take &= key != 0
    return key[take]


def default_takes_patches(n, S):
    """stats_use_patches without the knob: the average segment has at most SPP_MAXRUN pixels"""
    return n > 0 and n <= MAXRUN * (S + 1)


# ---- cases -----------------------------------------------------------------------------------------------------------
class Case(object):
    """name; entries: 'flat' (calcPerSegmentStats: the sorts) and/or 'patch' (the 2-D entry points); make() ->
    (seg (H, W) uint32, bands (nb, H, W), nulls [per band], S) and what the case wants to remember in .info"""

    def __init__(self, name, make, entries, missing=-9999, pcs=PCS, bands_extra=False):
        self.name, self._make, self.entries, self.missing, self.pcs = name, make, entries, missing, tuple(pcs)
        self.bands_extra = bands_extra              # also a four-band call
        self.info = {}

    def data(self):
        hit = _built.get(self.name)
        if hit is None:
            (seg, bands, nulls, S) = self._make(self)
            seg = np.ascontiguousarray(seg, dtype=np.uint32)
            bands = np.ascontiguousarray(bands)
            assert seg.ndim == 2 and bands.shape[1:] == seg.shape and len(nulls) == bands.shape[0]
            for a in (seg, bands):
                a.flags.writeable = False
            hit = (seg, bands, list(nulls), int(S))
            if seg.size > (1 << 20):
                _built.clear()                      # (one large raster at a time)
            _built[self.name] = hit
        return hit

    def sel(self):
        return selection(self.pcs)


_built = {}


def stride_order(n):
    """a fixed permutation of range(n): i -> i * P mod n, P a prime that does not divide n"""
    for P in (1000003, 999983, 7919, 7907):
        if math.gcd(P, n) == 1:
            return (np.arange(n, dtype=np.int64) * P) % n
    return np.arange(n, dtype=np.int64)


def linear(chunks, dtype, shuffle=True):
    """a 1 x N raster from (id, values) chunks, the pixels spread over the raster by stride_order"""
    seg = np.concatenate([np.full(len(v), i, dtype=np.uint32) for (i, v) in chunks])
    val = np.concatenate([np.asarray(v, dtype=np.int64) for (_i, v) in chunks])
    (lo, hi) = LIMITS[dtype]
    assert val.min() >= lo and val.max() <= hi
    if shuffle:
        order = stride_order(seg.size)
        (seg, val) = (seg[order], val[order])
    return seg[None, :], val.astype(dtype)[None, None, :]


def few_levels(n, salt):
    """n values on seven levels of uneven frequency (long runs of equal values once sorted)"""
    return (np.array([3, 3, 3, 10, 10, 500, 65000, 41])[mix(np.arange(n), salt) % 8]).astype(np.int64)


def all_distinct(n, salt):
    """n different values below 65535 (not the null value), in scrambled order"""
    v = stride_order(n) * 7 + salt
    assert v.max() < 65535
    return v


def _counts_case(counts, values, dtype='uint16', null=65535, nodata=None, zeros=0, S=None, above=0):
    """counts[id] valid pixels (id >= 1; counts[0] unused), nodata[id] null-valued ones, `zeros` pixels of the null
    segment and `above` pixels with ids above S"""
    S = len(counts) - 1 if S is None else S
    chunks = []
    for i in range(1, len(counts)):
        if counts[i]:
            chunks.append((i, values(counts[i], i)))
        if nodata is not None and nodata[i]:
            chunks.append((i, np.full(nodata[i], null, dtype=np.int64)))
    if zeros:
        chunks.append((0, few_levels(zeros, 99)))
    if above:
        chunks.append((S + 3, few_levels(above, 98)))
    (seg, bands) = linear(chunks, dtype)
    return seg, bands, [null], S


A1_SIZES = (1, 2, 63, 64, 65, STAGE - 1, STAGE, STAGE + 1, BIG - 1, BIG, BIG + 1,
            64 * (BIG // 64 + 1) - 1, 64 * (BIG // 64 + 1), 64 * (BIG // 64 + 1) + 1, 2 * BIG, 2 * BIG + 1)


def a1_ids():
    """the id of each size of A1_SIZES: 67 apart, in scrambled order, so that they fall into different wavefronts"""
    k = len(A1_SIZES)
    return [1 + ((j * 7) % k) * 67 for j in range(k)]


def _a1(values):
    def make(case):
        ids = a1_ids()
        S = max(ids) + 5
        counts = [0] + [1 + (i % 4) for i in range(1, S + 1)]
        for (i, n) in zip(ids, A1_SIZES):
            counts[i] = n
        nodata = [0] + [i % 3 for i in range(1, S + 1)]
        case.info['ids'] = dict(zip(A1_SIZES, ids))
        return _counts_case(counts, values, nodata=nodata)
    return make


def _a2(case):
    each = STAGE // 64
    assert each * 64 == STAGE and each <= BIG
    S = 5 * 64 + 10
    counts = [0] * (S + 1)
    nodata = [0] * (S + 1)
    for i in range(1, 64):
        counts[i] = 5 + i % 3
    for i in range(64, 128):                                  # wavefront 1: exactly STAGE values
        counts[i] = each
    for i in range(128, 192):                                 # wavefront 2: STAGE + 1
        counts[i] = each + (1 if i == 150 else 0)
    for i in range(192, 256):                                 # wavefront 3: a big segment among 63 small ones
        counts[i] = BIG + 1 if i == 200 else 2 + i % 5
    for i in range(256, 320):                                 # wavefront 4: no pixels / all nodata / ordinary
        (counts[i], nodata[i]) = ((0, 0), (0, 4), (6, 1))[i % 3]
    for i in range(320, S + 1):
        counts[i] = 3
    case.info.update(empty=[i for i in range(256, 320) if i % 3 == 0], allnull=[i for i in range(256, 320) if i % 3 == 1])
    return _counts_case(counts, few_levels, nodata=nodata, zeros=17)


def _a3(first_wave_full):
    def make(case):
        S = 40
        counts = [0] + [30 + i for i in range(1, S + 1)]
        assert sum(counts) <= STAGE
        if not first_wave_full:
            return _counts_case(counts, few_levels, null=65535)
        nodata = [0] + [STAGE // (2 * S) + 1] * S
        return _counts_case(counts, few_levels, nodata=nodata, zeros=STAGE // 2 + 1)
    return make


def _a4(S):
    def make(case):
        counts = [0] + [1 + i % 7 for i in range(1, S + 1)]
        counts[S] = 70
        return _counts_case(counts, few_levels, nodata=[0] + [i % 2 for i in range(1, S + 1)], above=9)
    return make


def runs(*pairs):
    """sorted values from (value, length) pairs, ascending in value"""
    assert all(a[0] < b[0] for (a, b) in zip(pairs, pairs[1:]))
    return np.repeat(np.array([p[0] for p in pairs], dtype=np.int64), [p[1] for p in pairs])


def a5_segments():
    """name -> the sorted values of a segment of more than SEGSTATS_BIG pixels"""
    n1 = BIG + 1
    steps = BIG // 64 + 1
    out = {}
    out['equal-big+1'] = runs((77, n1))
    out['equal-2big'] = runs((77, 2 * BIG))
    out['distinct'] = np.arange(n1, dtype=np.int64) + 11
    out['lane0'] = np.repeat(np.arange(steps, dtype=np.int64) * 3, 64)               # every boundary on lane 0
    out['runs63'] = np.repeat(np.arange(steps + 1, dtype=np.int64), 63)                # boundaries drift down the lanes
    out['runs65'] = np.repeat(np.arange(steps, dtype=np.int64), 65)                    # ... and up
    # ten single values, then one run over three steps that closes on lane 63, then single values
    out['close63'] = np.concatenate([np.arange(10), np.full(3 * 64 - 10, 10), np.arange(n1 - 3 * 64) + 11]).astype(np.int64)
    fill = BIG + 1 - 200
    (q, r) = divmod(fill, 7)
    sevens = [(100 + k, 7) for k in range(q)] + ([(100 + q, r)] if r else [])
    out['tie-two-longest'] = runs((5, 100), (9, 100), *sevens)                         # the smaller value wins
    out['longest-first'] = runs((5, 200), *sevens)
    out['longest-last'] = runs(*(sevens + [(60000, 200)]))                             # closed after the last step
    out['tie-last'] = runs((5, 100), *(sevens + [(60000, 100)]))                       # the last run only ties
    for (k, a) in out.items():
        assert a.size > BIG and (np.diff(a) >= 0).all(), k
    assert out['distinct'].size % 64 == 1 and out['lane0'].size % 64 == 0
    return out


def _a5(case):
    segs = a5_segments()
    chunks = []
    case.info['ids'] = {}
    for (k, (name, a)) in enumerate(sorted(segs.items())):
        i = 2 * k + 1
        case.info['ids'][name] = i
        chunks.append((i, a[stride_order(a.size)]))
        chunks.append((i + 1, few_levels(9, k)))
        chunks.append((i, np.full(k % 3, 65535)))
    (seg, bands) = linear(chunks, 'uint16')
    return seg, bands, [65535], 2 * len(segs)


def extreme_values(dtype, null, n, salt=0):
    """n values of dtype that hold both ends of its range (but for the null value) and their neighbours, the rest
    spread over the whole range"""
    (lo, hi) = LIMITS[dtype]
    width = hi - lo + 1
    v = lo + mix(np.arange(n), salt).astype(np.int64) % width
    ends = [lo, lo + 1, hi - 1, hi, lo, hi]
    v[:min(n, len(ends))] = ends[:min(n, len(ends))]
    if null is not None:
        v[v == null] = lo + 2
    return v


def _a6(dtype, null_end):
    def make(case):
        null = LIMITS[dtype][null_end]
        chunks = [(1, extreme_values(dtype, null, 40, 1)), (2, extreme_values(dtype, null, BIG + 1, 2)),
                  (1, np.full(3, null)), (2, np.full(5, null)), (3, np.full(4, null)),
                  (4, np.full(MAXRUN, LIMITS[dtype][1 - null_end]))]
        (seg, bands) = linear(chunks, dtype)
        return seg, bands, [null], 4
    return make


def _a7(case):
    nseg = BIG_WAVES + 1
    n = BIG + 1
    seg = np.repeat(np.arange(1, nseg + 1, dtype=np.uint32), n)
    val = (np.array([7, 7, 9, 300, 7], dtype=np.uint16))[(np.arange(seg.size, dtype=np.int64) * 3 // 2 + seg // 5) % 5]
    order = stride_order(seg.size)
    return seg[order][None, :], val[order][None, None, :], [None], nseg


def a8_plan():
    """(segment sizes, percentile parameters): every n <= SPP_MAXRUN that the scan names with all its p, five sizes up
    to SEGSTATS_BIG and three between SEGSTATS_BIG + 1 and 3 * SEGSTATS_BIG with one p each"""
    def pick(pairs, k):
        return pairs[::max(1, len(pairs) // k)][:k]
    small = percentile_float_pairs(1, MAXRUN + 1)
    mid = percentile_float_pairs(MAXRUN + 1, BIG + 1)
    chosen = small + [q for q in mid if q == (100, 7)] + pick(mid, 5) + pick(percentile_float_pairs(BIG + 1, 3 * BIG + 1), 3)
    sizes = sorted({n for (n, _p) in chosen})
    return sizes, sorted({p for (_n, p) in chosen} | set(PCS)), chosen


def _a8(case):
    (sizes, _pcs, chosen) = a8_plan()
    case.info['pairs'] = chosen
    case.info['ids'] = {n: i + 1 for (i, n) in enumerate(sizes)}
    chunks = [(i + 1, stride_order(n)) for (i, n) in enumerate(sizes)]          # values 0 .. n - 1: the column shows the index
    (seg, bands) = linear(chunks, 'uint16')
    return seg, bands, [65535], len(sizes)


def _a9(case):
    S = 70
    counts = [0] * (S + 1)
    nodata = [0] * (S + 1)
    for i in range(1, S + 1):
        (counts[i], nodata[i]) = ((5 + i % 4, 1), (0, 0), (0, 3), (2, 0))[i % 4]
    case.info.update(empty=[i for i in range(1, S + 1) if i % 4 == 1], allnull=[i for i in range(1, S + 1) if i % 4 == 2])
    return _counts_case(counts, few_levels, nodata=nodata, zeros=6, above=5)


# ---- patch cases: three bands with three null values --------------------------------------------------------------
def bands3(seg, dtype='uint16', salt=0, levels=37):
    """three planes of few levels (ties, modes) whose null values 0, 1, 2 fall on different pixels"""
    (H, W) = seg.shape
    i = np.arange(H * W).reshape(H, W)
    (lo, _hi) = LIMITS[dtype]
    planes = [(mix(i, salt * 3 + b) % levels).astype(np.int64) + lo for b in range(3)]
    return np.stack(planes).astype(dtype), [lo, lo + 1, lo + 2]


def block_labels(H, W, bh=4, bw=8, first=1):
    return ((np.arange(H)[:, None] // bh) * (-(-W // bw)) + np.arange(W)[None, :] // bw + first).astype(np.uint32)


B1_SHAPES = ((1, 1), (PH, PW), (PH - 1, PW - 1), (PH + 1, PW + 1), (1, 2 * PW * 16 + 1), (PH * PW + 1, 1))


def _b1(shape):
    def make(case):
        seg = block_labels(*shape)
        S = int(seg.max()) + 1                      # one label over the last row and column
        if shape[0] > 1:
            seg[-1, :] = S
        if shape[1] > 1:
            seg[:, -1] = S
        (bands, nulls) = bands3(seg, salt=shape[0])
        return seg, bands, nulls, int(seg.max())
    return make


def _b2(case):
    """patch 0: labels of 64 / 65 / 65-with-one-nodata pixels and an all-nodata one among 4 x 8 blocks; patches 1-3:
    one label each with exactly MAXRUN, MAXRUN + 1 and no valid pixels; patch 4: blocks"""
    seg = block_labels(PH, 5 * PW, first=10)
    flat0 = np.zeros(PATCH, dtype=np.uint32)
    sizes = [(1, MAXRUN), (2, MAXRUN + 1), (3, MAXRUN + 1), (4, 12)]
    at = 0
    for (i, n) in sizes:
        flat0[at:at + n] = i
        at += n
    p0 = seg[:, :PW].copy()
    p0.reshape(-1)[:at] = flat0[:at]
    seg[:, :PW] = p0
    for (k, i) in ((1, 5), (2, 6), (3, 7)):
        seg[:, k * PW:(k + 1) * PW] = i
    (bands, nulls) = bands3(seg, salt=2)
    b = bands.astype(np.int64)
    for k in range(3):
        b[k][np.isin(seg, (1, 2, 3, 4, 5, 6, 7)) & (b[k] == nulls[k])] = 20        # designed labels: nodata by hand only
    # band 0 is the band the table in the issue speaks of
    b[0][seg == 3] = np.where(np.arange((seg == 3).sum()) == 30, nulls[0], b[0][seg == 3])
    b[0][seg == 4] = nulls[0]
    for (i, nvalid) in ((5, MAXRUN), (6, MAXRUN + 1), (7, 0)):
        where = np.flatnonzero((seg == i).reshape(-1))
        keep = where[stride_order(where.size)[:nvalid]]
        plane = b[0].reshape(-1)
        vals = plane[keep].copy()
        plane[where] = nulls[0]
        plane[keep] = vals
    # the other bands: other valid counts of the same labels
    b[1][seg == 5] = np.where(np.arange(PATCH) < MAXRUN - 1, b[1][seg == 5], nulls[1])
    b[2][seg == 7] = np.where(np.arange(PATCH) < 1, 9, nulls[2])
    b[1][seg == 2] = np.where(np.arange(MAXRUN + 1) < 2, nulls[1], b[1][seg == 2])
    return seg, b.astype(np.uint16), nulls, int(seg.max())


def _b3(case):
    """2 x 2 patches; 64-pixel labels split 63 + 1 side by side (id 1), one above the other (id 2), and 61 + 1 + 1 + 1
    at the corner (id 3)"""
    seg = block_labels(2 * PH, 2 * PW, first=4)
    seg[5, 1:PW + 1] = 1                                                         # 63 left, 1 right
    seg[PH - 8:PH, PW + 36:PW + 44] = 2                                          # 8 x 8 above ...
    seg[PH - 8, PW + 36] = seg[PH - 9, PW + 36]                                  # ... less one ...
    seg[PH, PW + 36] = 2                                                         # ... and one below
    seg[PH - 1, PW - 61:PW] = 3
    seg[PH - 1, PW] = seg[PH, PW - 1] = seg[PH, PW] = 3
    for i in (1, 2, 3):
        assert (seg == i).sum() == MAXRUN
    (bands, nulls) = bands3(seg, salt=3)
    return seg, bands, nulls, int(seg.max())


B4_COUNTS = (MAXDIST - 1, MAXDIST, MAXDIST + 1, SLOTS, SLOTS + 1, PATCH)


def _b4(D):
    def make(case):
        seg = np.zeros((PH, 2 * PW), dtype=np.uint32)
        seg[:, :PW] = ((np.arange(PATCH, dtype=np.int64) * D) // PATCH + 1).reshape(PH, PW)
        seg[:, PW:] = block_labels(PH, PW, first=D + 1)
        (bands, nulls) = bands3(seg, salt=4)
        b = bands.astype(np.int64)
        b[0][:, :PW][b[0][:, :PW] == nulls[0]] = 30                              # band 0: every pixel of patch 0 valid
        return seg, b.astype(np.uint16), nulls, int(seg.max())
    return make


def _b5(case):
    """patch 0: 40 labels with one home slot among blocks; patch 1: six labels whose home is the last slot and two
    of the one before (the chain runs over the end of the table)"""
    crowd = ids_with_home(500, 40)
    tail = ids_with_home(SLOTS - 1, 6) + ids_with_home(SLOTS - 2, 2)
    seg = block_labels(PH, 2 * PW, first=1)
    taken = set(crowd) | set(tail)
    assert not taken & set(np.unique(seg).tolist())
    for (k, i) in enumerate(crowd):
        seg[k % PH, 8 * (k // PH):8 * (k // PH) + 8] = i
    for (k, i) in enumerate(tail):
        seg[2 * k, PW + 16:PW + 24] = i
    case.info.update(crowd=crowd, tail=tail)
    (bands, nulls) = bands3(seg, salt=5)
    return seg, bands, nulls, int(seg.max())


B6_RUNS = (1, 7, 8, 9, 15, 16, 17, MAXRUN - 1, MAXRUN)


def _b6(dtype):
    def make(case):
        (lo, hi) = LIMITS[dtype]
        lab = np.zeros(PATCH, dtype=np.uint32)
        val = np.zeros((3, PATCH), dtype=np.int64)
        nulls = [hi, lo, lo + 5]                                                # an end of the type, the other, neither
        at = 0
        ids = {}
        plan = [('run%d' % n, n) for n in B6_RUNS] + [('equal', MAXRUN), ('descending', MAXRUN), ('extremes', MAXRUN)]
        for (k, (name, n)) in enumerate(plan):
            ids[name] = k + 1
            lab[at:at + n] = k + 1
            for b in range(3):
                if name == 'equal':
                    v = np.full(n, lo + 7 + b)
                elif name == 'descending':
                    v = lo + 200 - np.arange(n) * 3 if dtype != 'uint8' else lo + 250 - np.arange(n) * 3
                elif name == 'extremes':
                    v = extreme_values(dtype, nulls[b], n, b)
                    v[n // 2] = nulls[b]                                        # (and one nodata pixel)
                else:
                    v = extreme_values(dtype, nulls[b], n, 10 + k + b) if k % 2 else lo + 6 + (mix(np.arange(n), k + b) % 5).astype(np.int64)
                val[b, at:at + n] = v
            at += n
        rest = np.arange(PATCH - at)
        lab[at:] = len(plan) + 1 + rest // 32
        for b in range(3):
            val[b, at:] = lo + 6 + (mix(rest, 50 + b) % 11).astype(np.int64)
        case.info['ids'] = ids
        return lab.reshape(PH, PW), val.reshape(3, PH, PW).astype(dtype), nulls, int(lab.max())
    return make


def _b7(case):
    """3 x 2 patches: a label of SEGSTATS_BIG + 1 pixels, 2-pixel labels across the patch boundary on every other row,
    complete blocks; flagged and unflagged ids alternate from id 2 on"""
    assert PH * 2 * PW == BIG
    seg = np.zeros((3 * PH, 2 * PW), dtype=np.uint32)
    seg[:PH] = block_labels(PH, 2 * PW, first=1)
    seg[2 * PH:] = block_labels(PH, 2 * PW, first=int(seg.max()) + 1)
    nblocks = int(seg.max())
    rows = [r for r in range(0, PH)] + [r for r in range(2 * PH + 1, 3 * PH)]
    strad = np.zeros_like(seg)
    for (k, r) in enumerate(rows):
        strad[r, PW - 1:PW + 1] = k + 1
    # ids: 1 = the big label; then straddlers on the even ids, blocks on the odd ones while the straddlers last
    new = np.zeros(nblocks + 1, dtype=np.uint32)
    blocks = np.unique(seg[seg != 0])
    new[blocks[:len(rows)]] = 3 + 2 * np.arange(len(rows))
    new[blocks[len(rows):]] = 2 + 2 * len(rows) + np.arange(len(blocks) - len(rows))
    out = new[seg]
    out[strad != 0] = 2 * strad[strad != 0]
    out[PH:2 * PH] = 1
    out[2 * PH, 0] = 1
    assert (out == 1).sum() == BIG + 1 and (out != 0).all()
    case.info.update(straddlers=[2 * (k + 1) for k in range(len(rows))])
    (bands, nulls) = bands3(out, salt=7)
    b = bands.astype(np.int64)
    b[0][(out == 1) & (b[0] == nulls[0])] = 20         # band 0: the big label keeps all its pixels (the wavefront path)
    return out, b.astype(np.uint16), nulls, int(out.max())


def _b7_complete(case):
    seg = block_labels(2 * PH, 2 * PW)
    (bands, nulls) = bands3(seg, salt=8)
    return seg, bands, nulls, int(seg.max())


def _b8(extra):
    def make(case):
        S = 31
        n = MAXRUN * (S + 1) + extra
        lab = np.minimum(np.arange(n) // MAXRUN, S).astype(np.uint32)           # MAXRUN pixels of label 0 first
        seg = lab[None, :]
        (bands, nulls) = bands3(seg, salt=9)
        return seg, bands, nulls, S
    return make


def _cases():
    # (the A cases are 1 x N rasters with their pixels spread out: through the 2-D entries nearly every label is left
    #  over, and the sorts run with the patch path's row filter at the same edges; A7 is kept to one call for its size)
    F, FP = ('flat',), ('flat', 'patch')
    out = [Case('A1-few-levels', _a1(few_levels), FP), Case('A1-all-distinct', _a1(all_distinct), FP),
           Case('A2-stage-limit', _a2, FP), Case('A3-first-wave-unstaged', _a3(True), FP),
           Case('A3-first-wave-staged', _a3(False), FP)]
    out += [Case('A4-S%d' % S, _a4(S), FP) for S in (62, 63, 64, 254, 255, 256)]
    out.append(Case('A5-run-structure', _a5, FP))
    out += [Case('A6-%s-null-%s' % (dt, ('min', 'max')[e]), _a6(dt, e), FP)
            for dt in ('uint8', 'int16', 'int32', 'uint32') for e in (0, 1)]
    out.append(Case('A7-second-trip', _a7, F, pcs=(0, 50)))
    out.append(Case('A8-percentiles', _a8, FP, pcs=a8_plan()[1]))
    out += [Case('A9-missing%d' % m, _a9, FP, missing=m) for m in (-9999, 7, -1)]
    out += [Case('B1-%dx%d' % s, _b1(s), FP) for s in B1_SHAPES]
    out += [Case('B2-completeness', _b2, FP), Case('B3-split-labels', _b3, FP)]
    out += [Case('B4-%d-labels' % D, _b4(D), FP) for D in B4_COUNTS]
    out.append(Case('B5-collisions', _b5, FP))
    out += [Case('B6-rank-%s' % dt, _b6(dt), FP, bands_extra=(dt == 'uint16'))
            for dt in ('uint8', 'int16', 'uint16', 'int32', 'uint32')]
    out += [Case('B7-both-paths', _b7, FP), Case('B7-nothing-left', _b7_complete, FP)]
    out += [Case('B8-default-at', _b8(0), FP), Case('B8-default-above', _b8(1), FP)]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def expected(case, orc):
    """[(intcols, floatcols) per band] of the oracle on the whole raster (read-only)"""
    (seg, bands, nulls, S) = case.data()
    out = []
    for (b, null) in enumerate(nulls):
        (ic, fc) = orc.segstats(seg, bands[b], case.sel(), null, case.missing, max_seg_id=S)
        ic.flags.writeable = False
        fc.flags.writeable = False
        out.append((ic, fc))
    return out


# ---- the GPU side (only called where there is one) -------------------------------------------------------------------
GUARD = 8                                       # words before and after the columns: they must keep their filler
GUARD_I64 = np.int64(-0x1111111111111112)       # 0xEEEE...EE
GUARD_U32 = np.uint32(0xEEEEEEEE)
KNOB = 'SHEPSEG_STATS_PATCH'


class _Knob(object):
    """SHEPSEG_STATS_PATCH = value ('1', '0') or unset (None) for the calls inside; the library reads it on every
    call"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get(KNOB)
        if self.value is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = self.old


def flat(seg, band, sel, null, missing, S):
    """tilingstats.calcPerSegmentStats: the shape is unknown there, so it never takes patches"""
    from pyshepseg_amd import tilingstats as ts
    (ic, fc, _fast) = ts.calcPerSegmentStats(seg.reshape(-1), band.reshape(-1), sel, imgNullVal=null,
                                             missingStatsValue=missing, maxSegId=S)
    return ic, fc


def _guarded(nint, nflt, ns):
    ibuf = np.full(nint * ns + 2 * GUARD, GUARD_I64, dtype=np.int64)
    fbuf = np.full(nflt * ns + 2 * GUARD, GUARD_U32, dtype=np.uint32)
    return ibuf, fbuf


def _unguard(ibuf, fbuf, nint, nflt, ns, tag):
    for (buf, word) in ((ibuf, GUARD_I64), (fbuf, GUARD_U32)):
        assert (buf[:GUARD] == word).all(), tag + ': words before the columns were written'
        assert (buf[buf.size - GUARD:] == word).all(), tag + ': words behind the columns were written'
    return (ibuf[GUARD:ibuf.size - GUARD].reshape(nint, ns), fbuf[GUARD:fbuf.size - GUARD].view(np.float32).reshape(nflt, ns))


class _Uploaded(object):
    """arrays in device memory for the calls inside (shp_dev_alloc + shp_dev_upload), freed on the way out"""

    def __init__(self, c, arrays):
        self.c, self.arrays, self.ptrs = c, arrays, []

    def __enter__(self):
        L = self.c._L
        try:
            for a in self.arrays:
                p = ctypes.c_void_p()
                self.c.check(L.shp_dev_alloc(self.c.handle, max(a.nbytes, 16), ctypes.byref(p)))
                self.ptrs.append(p)
                self.c.check(L.shp_dev_upload(self.c.handle, p, a.ctypes.data_as(ctypes.c_void_p), a.nbytes))
        except Exception:
            self.__exit__()
            raise
        return [p.value for p in self.ptrs]

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.c.check(self.c._L.shp_dev_free(self.c.handle, p))
        self.ptrs = []


def patch1(seg, band, sel, null, missing, S, knob):
    """shp_segstats2d_dev on device copies of seg (H, W) and band (H, W), SHEPSEG_STATS_PATCH = knob"""
    from pyshepseg_amd import _lib, tilingstats as ts
    c = _lib.ctx()
    (fast, ni, nf) = ts.makeFastStatsSelection(list(range(len(sel))), sel)
    (H, W) = seg.shape
    (ibuf, fbuf) = _guarded(ni, nf, S + 1)
    seg = np.ascontiguousarray(seg, dtype=np.uint32)
    band = np.ascontiguousarray(band)
    with _Knob(knob), _Uploaded(c, [seg, band]) as (d_seg, d_band):
        c.check(c._L.shp_segstats2d_dev(c.handle, d_seg, d_band, _lib.SHP_DTYPES[band.dtype], H, W, S,
                                        int(null is not None), 0 if null is None else int(null), _lib.ptr(fast),
                                        len(sel), int(missing), ctypes.c_void_p(ibuf.ctypes.data + 8 * GUARD),
                                        ctypes.c_void_p(fbuf.ctypes.data + 4 * GUARD)))
    return _unguard(ibuf, fbuf, ni, nf, S + 1, 'patch1 knob=%r' % knob)


def patchN(seg, bands, sel, nulls, missing, S, knob):
    """shp_segstats2d_bands_dev: the planes of `bands` with selection `sel` each; returns [(intcols, floatcols) per
    band] in the numbering of a one-band call"""
    from pyshepseg_amd import _lib, tilingstats as ts
    c = _lib.ctx()
    nb = len(bands)
    bandSelections = [(b + 1, [('b%d_%s' % (b, s[0]),) + tuple(s[1:]) for s in sel]) for b in range(nb)]
    (fast, bandOfStat, ni, nf) = ts.makeBandStatsSelection(bandSelections)
    (own, _oi, _of) = ts.makeFastStatsSelection(list(range(len(sel))), sel)
    (H, W) = seg.shape
    (ibuf, fbuf) = _guarded(ni, nf, S + 1)
    seg = np.ascontiguousarray(seg, dtype=np.uint32)
    planes = [np.ascontiguousarray(b) for b in bands]
    hasNull = np.array([int(v is not None) for v in nulls], dtype=np.int32)
    nullVal = np.array([0 if v is None else int(v) for v in nulls], dtype=np.int64)
    perBand = np.full(nb, len(sel), dtype=np.int32)
    with _Knob(knob), _Uploaded(c, [seg] + planes) as ptrs:
        table = (ctypes.c_void_p * nb)(*ptrs[1:])
        c.check(c._L.shp_segstats2d_bands_dev(c.handle, ptrs[0], table, _lib.SHP_DTYPES[planes[0].dtype], nb, H, W, S,
                                              _lib.ptr(hasNull), _lib.ptr(nullVal), _lib.ptr(fast), _lib.ptr(perBand),
                                              int(missing), ctypes.c_void_p(ibuf.ctypes.data + 8 * GUARD),
                                              ctypes.c_void_p(fbuf.ctypes.data + 4 * GUARD)))
    (ic, fc) = _unguard(ibuf, fbuf, ni, nf, S + 1, 'patchN bands=%d knob=%r' % (nb, knob))
    out = []
    for b in range(nb):
        rows = fast[bandOfStat == b]
        ints = [ic[r[3]] for (r, o) in zip(rows, own) if o[2] == 0]
        flts = [fc[r[3]] for (r, o) in zip(rows, own) if o[2] != 0]
        out.append((np.stack(ints), np.stack(flts)))
    return out
