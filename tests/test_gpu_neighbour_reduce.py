"""GPU: neighbours.reduceOverNeighbours against the numpy model (tests/neighbour_reduce_cases.py).

The exact cases use integer columns whose every partial sum stays below 2^53, so every summation order gives the
model's bits and numpy.array_equal holds for all nine statistics: they catch a lost, doubled or misattributed entry.
The thresholds of csrc/nbrreduce.h each have rows at T - 1, T and T + 1 entries (THRESHOLD_DEGREES): NBRR_LONG = 256
(the thread-per-row kernel hands the row to the wavefront-per-chunk kernel), NBRR_PIECE = 1024 (entries per LDS
piece) and NBRR_CHUNK = 4096 (entries per chunk of a long row; 2 * 4096 as well: a second chunk edge).  The span
case puts rows of 3 000, 70 000 and 300 000 entries between 100 000 short ones, so rows straddle every piece and
chunk edge.

Real-valued columns: the exact-type statistics equal the model; for the three float sums a row of n counted entries
must satisfy |got - exact| <= (n + 3) 2^-52 (sum w |x|) / sum w, the bound of n products, n - 1 additions, one
subtraction and one division in any order.  The model is the exact sum rounded once and divided once, within
2^-52 |model| of the exact value, so the tests ask |got - model| <= bound - 2^-52 |model|: no less than the bound."""
import ctypes
import functools

import numpy as np
import pytest

import aggregate_cases as ac
import neighbour_cases as nc
import neighbour_reduce_cases as rc
import table_cases as tc
from test_gpu_neighbours import find, in_fresh_context, real_raster, real_reference

pytestmark = pytest.mark.gpu

ALL = [(s, s) for s in rc.STATS]
FLOAT_SUMS = ('mean', 'bordermean', 'meanabsdiff')


@functools.lru_cache(maxsize=None)
def table(name):
    """(offsets, nbrs, lens, maxSegId), read-only"""
    if name == 'example':
        t = nc.reference_neighbours(nc.EXAMPLE, True)
    elif name == 'hot':
        t = nc.reference_neighbours(nc.hot_segment(), True)
    elif name == 'hot_top':
        t = nc.reference_neighbours(nc.hot_segment_top(), False)
    elif name == 'own8':
        t = nc.reference_neighbours(nc.every_pixel_its_own(), False)
    elif name == 'random1024':
        t = real_reference('random1024', False)
    elif name == 'mosaic':
        t = real_reference('mosaic', True)
    elif name == 'degrees':
        t = rc.table_with_degrees(rc.ISSUE_DEGREES, 21)[:3]
    elif name == 'thresholds':
        t = rc.table_with_degrees(rc.THRESHOLD_DEGREES, 22)[:3]
    else:
        assert name == 'span'
        t = rc.span_table()[:3]
    for a in t:
        a.setflags(write=False)
    return tuple(t) + (len(t[0]) - 2,)


TABLES = ['example', 'hot', 'hot_top', 'own8', 'random1024', 'mosaic', 'degrees', 'thresholds', 'span']


def handmade(name):
    from pyshepseg_amd import neighbours
    (offsets, nbrs, lens, maxSegId) = table(name)
    return neighbours.SegmentNeighbours(offsets, nbrs, lens, maxSegId, True)


def bound_of(name):
    """column magnitude of the exact cases: 2^20, and 2^10 on the span case whose rows reach 300 000 terms of
    w <= 2^10 (2^20 * 2^17 * 2^15 and 2^11 * 2^10 * 2^19 both stay below 2^53)"""
    return 1 << 10 if name == 'span' else 1 << 20


@functools.lru_cache(maxsize=None)
def integer_column(name):
    col = rc.integer_column(table(name)[3] + 1, bound_of(name), 31)
    col.setflags(write=False)
    return col


@functools.lru_cache(maxsize=None)
def integer_reference(name):
    (offsets, nbrs, lens, _m) = table(name)
    return rc.reference_reduce(offsets, nbrs, lens, integer_column(name))


@functools.lru_cache(maxsize=None)
def real_column(name):
    col = rc.real_column(table(name)[3] + 1, 32)
    col.setflags(write=False)
    return col


@functools.lru_cache(maxsize=None)
def real_model(name):
    (offsets, nbrs, lens, _m) = table(name)
    return rc.reference_reduce(offsets, nbrs, lens, real_column(name), withScales=True)


def reduce(nb, col, selection=ALL, **kw):
    from pyshepseg_amd import neighbours
    return neighbours.reduceOverNeighbours(nb, [(col, selection)], **kw)


def assert_equal(got, want, names=rc.STATS):
    for name in names:
        assert got[name].dtype == want[name].dtype == (np.int64 if name in rc.INT_STATS else np.float64), name
        assert got[name].shape == want[name].shape, name
        bad = np.flatnonzero(got[name] != want[name])
        assert len(bad) == 0, '%s: %d rows differ, the first %d: got %r, want %r' % (
            name, len(bad), bad[0], got[name][bad[0]], want[name][bad[0]])


def assert_same_bytes(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


# ---- 1: exact cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.int64], ids=['f64', 'f32', 'i64'])
@pytest.mark.parametrize('name', TABLES)
def test_exact(name, dtype):
    """the thresholds at T - 1, T, T + 1: NBRR_LONG 255 / 256 / 257, NBRR_PIECE 1023 / 1024 / 1025, NBRR_CHUNK 4095 /
    4096 / 4097 and 8191 / 8192 / 8193 ('degrees' and 'thresholds'); every integer of the columns is a float32"""
    nb = handmade(name)
    got = reduce(nb, integer_column(name).astype(dtype))
    assert sorted(got) == sorted(rc.STATS)
    assert_equal(got, integer_reference(name))
    assert nb.reduceTimings['uploaded'] and nb.reduceTimings['deviceMs'] > 0


def test_exact_cases_reach_every_path():
    deg = {name: np.diff(table(name)[0]) for name in TABLES}
    assert int(deg['hot'].max()) == int(deg['hot_top'].max()) == 22500 and int(deg['own8'].max()) == 8
    assert len(table('random1024')[1]) == 8352378
    for t in (rc.LONG, rc.PIECE, rc.CHUNK, 2 * rc.CHUNK):
        assert {t - 1, t, t + 1} <= set(deg['thresholds'].tolist())
    assert set(rc.ISSUE_DEGREES) <= set(deg['degrees'].tolist())
    assert set(rc.SPAN_LONG_ROWS) <= set(deg['span'].tolist())


# ---- 2: ties and signs ---------------------------------------------------------------------------------------
def test_nearest_ties_take_the_smallest_id():
    from pyshepseg_amd import neighbours
    # row 1: neighbours 2 (v 7) and 3 (v 3) around its own 5; row 4: 3 (v 3) and 5 (v -1) around its own 1; row 7: the
    # same two and 6 (v 1) at distance 0, which is no tie
    offsets = np.array([0, 0, 2, 2, 2, 4, 4, 4, 7], dtype=np.int64)
    nbrs = np.array([2, 3, 3, 5, 3, 5, 6], dtype=np.uint32)
    lens = np.array([1, 4, 2, 2, 2, 2, 9], dtype=np.int64)
    col = np.array([0, 5, 7, 3, 1, -1, 1, 1], dtype=np.float64)
    nb = neighbours.SegmentNeighbours(offsets, nbrs, lens, 7, True)
    got = reduce(nb, col)
    assert got['nearest'].tolist() == [0, 2, 0, 0, 3, 0, 0, 6]
    # strictly higher: the equal neighbour 6 of row 7 does not count
    assert got['bordertohigher'].tolist() == [0, 1, 0, 0, 2, 0, 0, 2]
    assert got['meanabsdiff'].tolist() == [-9999, 2, -9999, -9999, 2, -9999, -9999, 8 / 13]
    assert_equal(got, rc.reference_reduce(offsets, nbrs, lens, col))


@pytest.mark.parametrize('name', ['thresholds', 'mosaic'])
@pytest.mark.parametrize('value', [7.0, -3.5, 0.0])
def test_constant_column(name, value):
    """every distance ties: the nearest is the row's first (smallest) id, in short rows and across the lanes and
    chunks of long ones; nobody is higher"""
    (offsets, nbrs, lens, maxSegId) = table(name)
    col = np.full(maxSegId + 1, value)
    got = reduce(handmade(name), col)
    deg = np.diff(offsets)
    rows = np.flatnonzero(deg)
    assert np.array_equal(got['nearest'][rows], nbrs[offsets[rows]]) and not got['nearest'][deg == 0].any()
    assert not got['bordertohigher'].any() and (got['meanabsdiff'][rows] == 0).all()
    assert (got['mean'][rows] == value).all() and (got['min'][rows] == value).all()
    assert np.array_equal(got['count'], deg)
    assert_equal(got, rc.reference_reduce(offsets, nbrs, lens, col))


@pytest.mark.parametrize('name', ['degrees', 'hot_top'])
def test_negative_values(name):
    (offsets, nbrs, lens, maxSegId) = table(name)
    col = -1.0 - np.abs(integer_column(name))
    got = reduce(handmade(name), col)
    assert (got['max'][np.diff(offsets) > 0] < 0).all()
    assert_equal(got, rc.reference_reduce(offsets, nbrs, lens, col))


# ---- 3: ignored values ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def holed_column(name):
    """the integer column with -9999 in a third of the rows, and in every neighbour of the first row that has any"""
    (offsets, nbrs, _lens, maxSegId) = table(name)
    col = np.array(integer_column(name))
    col[np.random.default_rng(33).random(maxSegId + 1) < 1.0 / 3.0] = -9999
    r = int(np.flatnonzero(np.diff(offsets))[0])
    col[nbrs[offsets[r]:offsets[r + 1]]] = -9999
    col.setflags(write=False)
    return col


@pytest.mark.parametrize('name', ['degrees', 'mosaic', 'span'])
def test_ignore_value(name):
    (offsets, nbrs, lens, maxSegId) = table(name)
    col = holed_column(name)
    want = rc.reference_reduce(offsets, nbrs, lens, col, ignoreValue=-9999)
    deg = np.diff(offsets)
    emptied = (deg > 0) & (want['count'] == 0)
    ownless = (col == -9999) & (want['count'] > 0)
    assert emptied.any() and ownless.any() and (want['count'] < deg).any()
    got = reduce(handmade(name), col, ignoreValue=-9999)
    assert_equal(got, want)
    for stat in ('min', 'max', 'mean', 'bordermean', 'meanabsdiff'):
        assert (got[stat][emptied] == -9999).all()
    assert (got['meanabsdiff'][ownless] == -9999).all()
    for stat in rc.INT_STATS:
        assert not got[stat][emptied].any()
    assert not got['nearest'][ownless].any() and not got['bordertohigher'][ownless].any()
    assert got['border'][ownless].all()
    # without the ignore value -9999 is a value like any other
    assert_equal(reduce(handmade(name), col), rc.reference_reduce(offsets, nbrs, lens, col))


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('name', ['degrees', 'mosaic'])
def test_nan_is_ignored_and_missing_value(name, dtype):
    (offsets, nbrs, lens, maxSegId) = table(name)
    col = holed_column(name).astype(dtype)
    col[col == -9999] = np.nan
    want = rc.reference_reduce(offsets, nbrs, lens, col, missing=-1.5)
    assert_equal(want, rc.reference_reduce(offsets, nbrs, lens, holed_column(name), ignoreValue=-9999, missing=-1.5))
    got = reduce(handmade(name), col, missingStatsValue=-1.5)
    assert_equal(got, want)
    assert (got['mean'][want['count'] == 0] == -1.5).all()
    # NaN stays ignored beside an ignore value
    col2 = np.array(col)
    col2[3] = 12345
    assert_equal(reduce(handmade(name), col2, ignoreValue=12345, missingStatsValue=7),
                 rc.reference_reduce(offsets, nbrs, lens, col2, ignoreValue=12345, missing=7))


# ---- 4: real-valued columns ----------------------------------------------------------------------------------
def assert_within_bound(got, model):
    n = model['n']
    have = n > 0
    for stat in FLOAT_SUMS:
        tol = (n + 3) * 2.0 ** -52 * model['scale:' + stat] - 2.0 ** -52 * np.abs(model[stat])
        err = np.abs(got[stat] - model[stat])
        worst = int(np.argmax(np.where(have, err - tol, -np.inf)))
        print('%s: largest error %.3g, row %d has error %.3g of a bound %.3g (n = %d)' % (
            stat, err[have].max(), worst, err[worst], tol[worst], n[worst]))
        assert (err[have] <= tol[have]).all(), stat
        assert (got[stat][~have] == model[stat][~have]).all(), stat


@pytest.mark.parametrize('name', ['span', 'random1024'])
def test_real_valued_columns(name):
    model = real_model(name)
    got = reduce(handmade(name), real_column(name))
    assert_equal(got, model, ('count', 'border', 'min', 'max', 'bordertohigher', 'nearest'))
    assert_within_bound(got, model)


# ---- 5: the order depends on the row alone ----------------------------------------------------------------------
def test_same_bytes_resident_and_uploaded():
    from pyshepseg_amd import neighbours
    col = real_column('random1024')
    nb = find(real_raster('random1024'), False)
    assert nb.residentSerial is not None and nb.residentSerial == neighbours.residentTableSerial()
    first = reduce(nb, col)
    assert not nb.reduceTimings['uploaded'] and nb.reduceTimings['upload'] == 0.0
    again = reduce(nb, col)
    assert not nb.reduceTimings['uploaded']
    assert_same_bytes(first, again)
    serial = nb.residentSerial
    other = find(nc.EXAMPLE, True)
    assert neighbours.residentTableSerial() == other.residentSerial != serial == nb.residentSerial
    uploaded = reduce(nb, col)
    assert nb.reduceTimings['uploaded'] and nb.reduceTimings['upload'] > 0
    assert nb.residentSerial == neighbours.residentTableSerial() not in (serial, other.residentSerial)
    assert_same_bytes(first, uploaded)
    byhand = handmade('random1024')
    assert byhand.residentSerial is None
    assert_same_bytes(first, reduce(byhand, col))
    assert byhand.reduceTimings['uploaded'] and byhand.residentSerial == neighbours.residentTableSerial()
    # the table that was pushed out comes back by upload, too
    assert reduce(other, np.array([0.0, 10.0, 4.0, 7.0]))['nearest'].tolist() == [0, 3, 3, 1]
    assert other.reduceTimings['uploaded']
    assert_within_bound(first, real_model('random1024'))


def test_same_bytes_span_twice():
    col = real_column('span')
    nb = handmade('span')
    first = reduce(nb, col)
    assert nb.reduceTimings['uploaded']
    again = reduce(nb, col)
    assert not nb.reduceTimings['uploaded']
    assert_same_bytes(first, again)
    assert_same_bytes(first, reduce(handmade('span'), col))


def test_a_row_in_two_tables():
    """the span case's long rows and three short ones keep their entries in a table whose other rows differ: they
    start elsewhere in the arrays and share workgroups, pieces and launches with other rows"""
    from pyshepseg_amd import neighbours
    (offsets, nbrs, lens, maxSegId) = table('span')
    deg = np.diff(offsets)
    short = [int(r) for r in np.flatnonzero((deg >= 5) & (deg <= rc.LONG))[[0, 700, -1]]]
    keep = [50000, 50001, 50002] + short
    deg2 = np.random.default_rng(77).geometric(1.0 / 4.0, size=100000).astype(np.int64) - 1
    deg2[np.array(keep) - 1] = deg[keep]
    (offsets2, nbrs2, lens2, maxSegId2) = rc.table_with_degrees(deg2, 78, maxLength=1 << 10)
    assert maxSegId2 == maxSegId
    for r in keep:
        assert offsets2[r] != offsets[r]
        nbrs2[offsets2[r]:offsets2[r + 1]] = nbrs[offsets[r]:offsets[r + 1]]
        lens2[offsets2[r]:offsets2[r + 1]] = lens[offsets[r]:offsets[r + 1]]
    assert rc.table_violations(offsets2, nbrs2, lens2) == []
    col = real_column('span')
    a = reduce(handmade('span'), col)
    b = reduce(neighbours.SegmentNeighbours(offsets2, nbrs2, lens2, maxSegId2, True), col)
    for stat in rc.STATS:
        assert a[stat][keep].tobytes() == b[stat][keep].tobytes(), stat
    assert not all(a[stat].tobytes() == b[stat].tobytes() for stat in FLOAT_SUMS)


# ---- 5b: three owners of a list of long rows in one context -----------------------------------------------------
LISTS_S = rc.LONG + 3
LISTS_STATS = ('mean', 'bordermean', 'nearest')


@functools.lru_cache(maxsize=None)
def list_tables():
    """(T1, T2, T3) over the ids 0 .. LONG + 3: a star of LONG + 2 leaves around id 1, the same star around the last
    id, and a chain; lengths 1 .. 9"""
    S = LISTS_S
    leaves = np.arange(2, S + 1, dtype=np.int64)
    w = 1 + np.arange(len(leaves)) % 9
    t1 = tc.table_from_edges(S, np.ones(len(leaves), dtype=np.int64), leaves, w)
    t2 = tc.table_from_edges(S, leaves - 1, np.full(len(leaves), S, dtype=np.int64), w)
    i = np.arange(1, S, dtype=np.int64)
    t3 = tc.table_from_edges(S, i, i + 1, 1 + i % 9)
    return (t1, t2, t3)


def long_rows(table):
    return np.flatnonzero(np.diff(table[0]) > rc.LONG).tolist()


def test_list_tables_have_their_long_rows():
    """no GPU: one row above NBRR_LONG in T1 and in T2, at different indices, none in T3; the share of T2 that holds
    the hub lists it at another index again; one chunk each"""
    (t1, t2, t3) = list_tables()
    assert (long_rows(t1), long_rows(t2), long_rows(t3)) == ([1], [LISTS_S], [])
    assert int(np.diff(t1[0]).max()) == int(np.diff(t2[0]).max()) == rc.LONG + 2 <= rc.CHUNK
    share = tc.share_of(t2, 1, 2)
    (lo, hi) = share.idRange
    assert lo > 1 and hi == LISTS_S + 1 and long_rows((share.offsets,)) == [LISTS_S - lo]


def test_long_row_lists_of_two_tables_and_a_member_list_interleaved():
    """One context, one thread: reductions over T1, T2, T3 (each upload a new table), over the share of T2 that holds
    the hub, an aggregation over a member list with one long row, then T1 and the share again.  Each owner of a list
    of long rows must use its own, rebuilt exactly when its table changed: every result equals the numpy model bit
    for bit (integer columns: exact in any order)."""
    import types
    from pyshepseg_amd import _lib, distributed, neighbours
    from pyshepseg_amd import comm as shpcomm
    tables = list_tables()
    col = rc.integer_column(LISTS_S + 1, 1 << 20, 41)
    selection = [(s, s) for s in LISTS_STATS]
    want = [rc.reference_reduce(*t, col, stats=LISTS_STATS) for t in tables]
    recode = np.ones(LISTS_S + 1, dtype=np.uint32)
    recode[0] = 0
    assert long_rows(ac.member_csr(recode, 1)) == [1]
    aggStats = [(s, s) for s in ac.STATS]
    aggWant = ac.reference_aggregate(recode, 1, col)

    def same_bits(got, model, rows=slice(None)):
        assert sorted(got) == sorted(LISTS_STATS)
        for name in LISTS_STATS:
            assert got[name].dtype == model[name].dtype, name
            assert got[name][rows].tobytes() == model[name][rows].tobytes(), name

    def steps():
        c = _lib.ctx()
        (engine, comm) = (types.SimpleNamespace(c=c), shpcomm.LocalComm())
        whole = [tc.whole_of(t) for t in tables]
        for k in (0, 1, 2):                                                            # steps 1 to 3
            same_bits(reduce(whole[k], col, selection), want[k])
            assert whole[k].reduceTimings['uploaded']
        share = tc.share_of(tables[1], 1, 2)
        rows = slice(*share.idRange)
        got = distributed.reduceOverNeighboursDistributed(engine, comm, share, [(col, selection)])       # step 4
        assert share.reduceTimings['uploaded']
        same_bits(got, want[1], rows)
        byHand = neighbours.MergedSegments()                                            # step 5
        (byHand.recode, byHand.maxSegId) = (recode, 1)
        agg = neighbours.aggregateToGroups(byHand, [(col, aggStats)])
        for name in ac.STATS:
            assert agg[name].dtype == aggWant[name].dtype and np.array_equal(agg[name], aggWant[name]), name
        same_bits(reduce(whole[0], col, selection), want[0])                            # step 6
        assert whole[0].reduceTimings['uploaded']
        got = distributed.reduceOverNeighboursDistributed(engine, comm, share, [(col, selection)])       # step 7
        assert not share.reduceTimings['uploaded']
        same_bits(got, want[1], rows)
    in_fresh_context(steps)


# ---- 6: several columns, shared output ---------------------------------------------------------------------------
def test_several_columns_in_one_call():
    from pyshepseg_amd import neighbours
    nb = handmade('mosaic')
    n = nb.maxSegId + 1
    cols = [real_column('mosaic'), integer_column('mosaic').astype(np.float32), integer_column('mosaic').astype(np.int64) // 3]
    picks = [[('b1_mean', 'mean'), ('b1_near', 'nearest'), ('b1_n', 'count')],
             [('b2_mean', 'mean'), ('b2_mad', 'meanabsdiff'), ('b2_bm', 'bordermean'), ('b2_mean_again', 'mean')],
             [('b3_n', 'count'), ('b3_high', 'bordertohigher'), ('b3_min', 'min'), ('b3_max', 'max'), ('b3_b', 'border')]]
    together = neighbours.reduceOverNeighbours(nb, list(zip(cols, picks)), ignoreValue=0)
    assert sorted(together) == sorted(name for pick in picks for (name, _s) in pick)
    for (col, pick) in zip(cols, picks):
        alone = neighbours.reduceOverNeighbours(nb, [(col, pick)], ignoreValue=0)
        assert sorted(alone) == sorted(name for (name, _s) in pick)
        for name in alone:
            assert together[name].tobytes() == alone[name].tobytes() and together[name].dtype == alone[name].dtype
    assert together['b2_mean'].tobytes() == together['b2_mean_again'].tobytes()
    assert together['b2_mean'] is not together['b2_mean_again']
    # beside the statistics' columns and the table's own
    columns = {'Histogram': np.ones(n, dtype=np.int64)}
    columns.update(nb.columns)
    columns.update(together)
    assert all(len(c) == n for c in columns.values()) and len(columns) == 3 + len(together)
    assert np.array_equal(columns['b3_n'] <= columns['numNeighbours'], np.ones(n, dtype=bool))


# ---- 7: upload validation, call order ---------------------------------------------------------------------------
def broken_example(which, index, value):
    from pyshepseg_amd import neighbours
    arrays = [np.array(a) for a in table('example')[:3]]
    for (w, i, v) in zip(np.atleast_1d(which), np.atleast_1d(index), np.atleast_1d(value)):
        arrays[w][i] = v
    return neighbours.SegmentNeighbours(arrays[0], arrays[1], arrays[2], 3, True)


VIOLATIONS = [((0, 1, 1), 'first', 'offset 1: offsets\\[0\\] and offsets\\[1\\] must be 0'),
              ((0, 3, 1), 'decreasing', 'offset 3: the offsets must not decrease'),
              ((0, 4, 7), 'end', 'offset 4: the last offset must be the number of entries'),
              ((1, 1, 9), 'range', 'entry 1: a neighbour id outside 1..max_seg_id'),
              ((1, 3, 2), 'self', 'entry 3: a row names itself'),
              ((1, 1, 2), 'order', 'entry 1: the ids of a row must ascend strictly'),
              ((2, 4, 0), 'length', 'entry 4: a border length below 1'),
              (([2, 1], [4, 1], [0, 2]), 'order', 'entry 1: the ids of a row must ascend strictly'),
              (([2, 0], [0, 3], [-5, 1]), 'decreasing', 'offset 3: the offsets must not decrease')]


@pytest.mark.parametrize('change,rule,message', VIOLATIONS, ids=[str(i) for i in range(len(VIOLATIONS))])
def test_upload_refuses_a_broken_table(change, rule, message):
    from pyshepseg_amd import _lib, neighbours
    col = np.array([0.0, 10.0, 4.0, 7.0])

    def attempt():
        nb = broken_example(*change)
        assert rule in rc.table_violations(nb.offsets, nb.neighbours, nb.borderLengths)
        good = handmade('example')
        assert reduce(good, col)['nearest'].tolist() == [0, 3, 3, 1]
        assert neighbours.residentTableSerial() == good.residentSerial
        with pytest.raises(neighbours.PyShepSegNeighboursError, match='not a neighbour table: ' + message):
            reduce(nb, col)
        # no finished table is left, not even the one before
        assert neighbours.residentTableSerial() is None and nb.residentSerial is None
        c = _lib.ctx()
        out = np.zeros(4)
        ptrs = (ctypes.c_void_p * 9)()
        ptrs[4] = out.ctypes.data
        assert c._L.shp_nbr_reduce(c.handle, _lib.ptr(col), 0, 4, 0, 0.0, -9999.0, 1 << 4, ptrs, None) != 0
        assert 'no finished table' in c._L.shp_last_error(c.handle).decode()
        assert reduce(good, col)['nearest'].tolist() == [0, 3, 3, 1] and good.reduceTimings['uploaded']
    in_fresh_context(attempt)


def test_upload_finds_a_violation_inside_a_long_row():
    from pyshepseg_amd import neighbours
    (offsets, nbrs, lens, maxSegId) = table('thresholds')
    r = 1 + rc.THRESHOLD_DEGREES.index(2 * rc.CHUNK + 1)
    nbrs = np.array(nbrs)
    lens = np.array(lens)
    e = int(offsets[r]) + 5000
    nbrs[e] = nbrs[e - 1]
    lens[e + 100] = 0
    nb = neighbours.SegmentNeighbours(offsets, nbrs, lens, maxSegId, True)
    with pytest.raises(neighbours.PyShepSegNeighboursError, match='entry %d: the ids of a row must ascend strictly' % e):
        in_fresh_context(lambda: reduce(nb, integer_column('thresholds')))


def test_reduce_needs_a_finished_table():
    """refused on the host side of the C call, before any kernel"""
    from pyshepseg_amd import _lib, neighbours

    def calls():
        c = _lib.ctx()
        L = c._L
        col = np.array([0.0, 10.0, 4.0, 7.0])
        out = np.full(4, 5.0)
        ptrs = (ctypes.c_void_p * 9)()
        ptrs[4] = out.ctypes.data

        def refused():
            assert L.shp_nbr_reduce(c.handle, _lib.ptr(col), 0, 4, 0, 0.0, -9999.0, 1 << 4, ptrs, None) == -5
            assert 'no finished table' in L.shp_last_error(c.handle).decode()
            assert out.tolist() == [5.0] * 4 and neighbours.residentTableSerial() is None
        refused()
        c.check(L.shp_nbr_begin(c.handle, 3, 1))
        refused()
        (S, nent, bad) = (ctypes.c_uint32(0), ctypes.c_int64(0), ctypes.c_uint32(0))
        c.check(L.shp_nbr_finish(c.handle, ctypes.byref(S), ctypes.byref(nent), ctypes.byref(bad), None, None))
        assert (S.value, nent.value) == (3, 0) and neighbours.residentTableSerial() is not None
        c.check(L.shp_nbr_reduce(c.handle, _lib.ptr(col), 0, 4, 0, 0.0, -9999.0, 1 << 4, ptrs, None))
        assert out.tolist() == [-9999.0] * 4
        # arguments the C call refuses itself
        assert L.shp_nbr_reduce(c.handle, _lib.ptr(col), 0, 5, 0, 0.0, -9999.0, 1 << 4, ptrs, None) == -3
        assert L.shp_nbr_reduce(c.handle, _lib.ptr(col), 3, 4, 0, 0.0, -9999.0, 1 << 4, ptrs, None) == -3
        assert L.shp_nbr_reduce(c.handle, _lib.ptr(col), 0, 4, 0, 0.0, -9999.0, 1 << 5, ptrs, None) == -3
        assert L.shp_nbr_reduce(c.handle, _lib.ptr(col), 0, 4, 0, 0.0, -9999.0, 0, ptrs, None) == -3
        # a new begin takes the finished table away again (out: what a refused call must leave alone)
        out[:] = 5.0
        c.check(L.shp_nbr_begin(c.handle, 3, 1))
        refused()
        return True
    assert in_fresh_context(calls)


# ---- 8: degenerate tables ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('maxSegId', [0, 9])
def test_tables_without_entries(maxSegId):
    from pyshepseg_amd import neighbours
    n = maxSegId + 1
    nb = neighbours.SegmentNeighbours(np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.uint32),
                                      np.zeros(0, dtype=np.int64), maxSegId, True)
    resident = find(np.zeros((40, 70), dtype=np.uint32), True, maxSegId=maxSegId)
    for t in (nb, resident):
        for dtype in (np.float64, np.float32, np.int64):
            got = reduce(t, np.arange(n).astype(dtype), missingStatsValue=2.5)
            assert sorted(got) == sorted(rc.STATS)
            for stat in rc.STATS:
                assert got[stat].shape == (n,)
                assert got[stat].tolist() == [0 if stat in rc.INT_STATS else 2.5] * n
    assert not resident.reduceTimings['uploaded'] and nb.reduceTimings['uploaded'] is False
