"""The shared prefix sum (csrc/scan.h) and radix sort (csrc/sort.h) on their own, through shp_prim_scan /
shp_prim_sort, against their numpy definitions at the block and digit edges (cases and models: tests/prim_cases.py;
what the case lists reach is counted in tests/test_prim_cases_host.py).  Integer work: numpy.array_equal throughout.

Every output lies between guard words that must keep their filler, the scan's two totals (the device word and the
word mirrored into pinned memory) are checked separately, and a one-pass sort also hands back its 257 digit starts as
the k-means fit reads them (sort_digit_start)."""
import ctypes

import numpy as np
import pytest

import prim_cases as pc

pytestmark = pytest.mark.gpu

SHP_ERR_ARG = -3


@pytest.fixture(scope='module')
def dev():
    d = pc.Dev()
    yield d
    d.close()


_scan_want = {}


def scan_want(case):
    """(input, expected output, expected total) of a case, computed once and read-only"""
    key = (case.content, case.n)
    if key not in _scan_want:
        a = case.data()
        out, total = pc.scan_model(a)
        out.flags.writeable = False
        _scan_want[key] = (a, out, total)
    return _scan_want[key]


def check_scan(dev, d_in, n, want, total, skew_in=0, skew_out=0, flags=pc.SCAN_FLAGS, out='scan_out'):
    """shp_prim_scan of the n words at d_in under each (get4, lazy) of flags; returns the last run's record"""
    r = None
    for get4, lazy in flags:
        tag = 'scan n=%d get4=%d lazy=%d skew_in=%d skew_out=%d: ' % (n, get4, lazy, skew_in, skew_out)
        r = dev.scan(d_in, n, get4, lazy, skew_out, out)
        assert r['clean'], tag + 'words outside the output or the block offsets were written'
        if lazy:
            assert r['nboff'] == pc.scan_lazy_count(n), tag + 'block offsets handed back'
        diff = pc.first_diff(pc.scan_lazy_apply(r['out_raw'], r['boff']), want)
        assert not diff, tag + diff
        assert r['total_dev'] == total, tag + 'the device total'
        assert r['total_mirror'] == total, tag + 'the mirrored total'
    return r


@pytest.mark.parametrize('case', [c for c in pc.SCAN_CASES if c.n != pc.SCAN_BIG], ids=lambda c: c.name)
def test_scan_case(dev, case):
    a, want, total = scan_want(case)
    d_in = dev.upload('scan_in', a, case.skew_in)
    check_scan(dev, d_in, case.n, want, total, case.skew_in, case.skew_out)


def test_scan_two_levels(dev):
    """SCAN_ITEMS^2 + 1 items: the top level stores its block totals plainly and a second, one-launch scan of
    SCAN_ITEMS + 1 totals (scratch behind the first level's) makes the offsets.  Skipped only when the device has no
    room for the two buffers."""
    (case,) = [c for c in pc.SCAN_CASES if c.n == pc.SCAN_BIG]
    try:
        dev.buf('big_in', case.n + 4)
        dev.buf('big_out', case.n + 2 * pc.GUARD + 4)
    except pc.AllocRefused as e:
        dev.release('big_in')
        pytest.skip('no device memory for %s' % e)
    try:
        a = case.data()
        want, total = pc.scan_model(a)
        d_in = dev.upload('big_in', a)
        check_scan(dev, d_in, case.n, want, total, out='big_out')
    finally:
        dev.release('big_in')
        dev.release('big_out')


_sort_want = {}


def sort_want(case):
    key = (case.n, case.bits, case.content, case.has_vals)
    if key not in _sort_want:
        if len(_sort_want) > 8:
            _sort_want.clear()
        keys, vals = case.keys(), case.vals()
        _sort_want[key] = (keys, vals) + pc.sort_model(keys, vals, case.bits) + (pc.digit_starts_model(keys),)
    return _sort_want[key]


@pytest.mark.parametrize('case', pc.SORT_CASES, ids=lambda c: c.name)
def test_sort_case(dev, case):
    keys, vals, kwant, vwant, swant = sort_want(case)
    tag = 'sort %s (n=%d bits=%d staged=%d values=%s keys wanted=%d): ' % (
        case.name, case.n, case.bits, case.staged, 'given' if case.has_vals else 'index', case.want_keys)
    r = dev.sort(keys, vals, case.bits, case.staged, case.want_keys)
    assert r['clean'], tag + 'words outside the outputs were written'
    diff = pc.first_diff(r['vals_out'], vwant)
    assert not diff, tag + 'values: ' + diff
    if case.want_keys:
        diff = pc.first_diff(r['keys_out'], kwant)
        assert not diff, tag + 'keys: ' + diff
    if case.passes == 1:
        diff = pc.first_diff(r['starts'], swant)
        assert not diff, tag + 'digit starts: ' + diff


def test_counter_and_workspace_hygiene(dev):
    """forty scans in one context, multi-block one-launch and one-block in turn, with and without get4: a ticket
    counter left non-zero breaks the next multi-block scan.  Then a sort, then the product's segment locations: it
    still finds its workspaces in order."""
    many = pc.ScanCase('many', 3 * pc.SCAN_ITEMS + pc.SCAN_SUB - 3, 'random')
    one = pc.ScanCase('one', pc.SCAN_SUB + 1, 'random')
    assert 1 < pc.scan_blocks(many.n) <= pc.SCAN_ITEMS and pc.scan_blocks(one.n) == 1
    d_many, d_one = dev.upload('hyg_many', many.data()), dev.upload('hyg_one', one.data())
    for i in range(40):
        case, d_in = ((many, d_many), (one, d_one))[i % 2]
        a, want, total = scan_want(case)
        check_scan(dev, d_in, case.n, want, total, flags=(((i // 2) % 2 == 0, (i // 4) % 2 == 1),))
    case = pc.SortCase(pc.HIST_BLOCKS * pc.SORT_TILE + 1, 17, 'random', True, True, True)
    keys, vals = case.keys(), case.vals()
    r = dev.sort(keys, vals, case.bits, case.staged, True)
    kwant, vwant = pc.sort_model(keys, vals, case.bits)
    assert r['clean'] and np.array_equal(r['keys_out'], kwant) and np.array_equal(r['vals_out'], vwant)
    rng = np.random.RandomState(3)
    seg = rng.randint(0, 41, size=(37, 53)).astype(np.uint32)
    off = np.zeros(42, dtype=np.uint32)
    pix = np.empty(seg.size, dtype=np.uint32)
    c = dev.c
    c.check(c._L.shp_segment_locations(c.handle, seg.ctypes.data_as(ctypes.c_void_p), 37, 53, 40,
                                       off.ctypes.data_as(ctypes.c_void_p), pix.ctypes.data_as(ctypes.c_void_p)))
    assert np.array_equal(off, np.r_[0, np.cumsum(np.bincount(seg.ravel(), minlength=41))])
    assert np.array_equal(pix, np.argsort(seg.ravel(), kind='stable'))
    a, want, total = scan_want(many)
    check_scan(dev, d_many, many.n, want, total)           # and the scan after the product's own calls


def test_scan_of_a_scan(dev):
    """three scans deep, each reading what the one before wrote"""
    n = 2 * pc.SCAN_ITEMS + 1
    a = pc.random_words(n, 'scan')
    d_in = dev.upload('chain_in', a)
    for depth in range(3):
        want, total = pc.scan_model(a)
        out = 'chain_%d' % (depth % 2)
        r = check_scan(dev, d_in, n, want, total, flags=((depth != 1, False),), out=out)
        a, d_in = want, r['d_out']


@pytest.mark.parametrize('n', (1, pc.SORT_TILE + 1, pc.HIST_BLOCKS * pc.SORT_TILE + 1, 200003))
@pytest.mark.parametrize('k', (2, 60, 256))
def test_digit_starts_of_cluster_labels(dev, k, n):
    """what the k-means fit does: labels below k sorted in one pass (bits_for(k - 1)), the clusters' ranges read from
    the pass's scanned histogram.  Some clusters are empty, the first and the last among them.  The staged form keeps
    the same histogram layout (digit-major, one column per block), so it is held to the same starts."""
    rng = np.random.RandomState(1000 * k + n % 997)
    if k == 2:
        variants = [np.zeros(n, dtype=np.uint32), np.ones(n, dtype=np.uint32)]       # the last empty; the first empty
    else:
        live = np.arange(1, k - 1)[rng.rand(k - 2) < 0.7]                  # neither 0 nor k - 1, and gaps between
        variants = [live[rng.randint(0, live.size, size=n)].astype(np.uint32)]
    bits = max(1, int(k - 1).bit_length())
    assert pc.sort_passes(bits) == 1
    for keys in variants:
        want = pc.digit_starts_model(keys)
        kwant, vwant = pc.sort_model(keys, None, bits)
        for staged in (False, True):
            tag = 'digit starts k=%d n=%d staged=%d: ' % (k, n, staged)
            r = dev.sort(keys, None, bits, staged, True)
            st = r['starts']
            diff = pc.first_diff(st, want)
            assert not diff, tag + diff
            assert np.array_equal(r['keys_out'], kwant) and np.array_equal(r['vals_out'], vwant), tag + 'the sort'
            # and they are consistent with the sorted keys: cluster d's rows are [st[d], st[d + 1])
            assert st[0] == 0 and st[256] == n and (np.diff(st.astype(np.int64)) >= 0).all(), tag
            assert np.array_equal(np.repeat(np.arange(256), np.diff(st.astype(np.int64))), r['keys_out']), tag


def test_entry_points_refuse_bad_arguments(dev):
    c, L = dev.c, dev.L
    d = dev.buf('args', 16)
    tot, mir, nb = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()

    def refused(rc, text):
        assert rc == SHP_ERR_ARG and L.shp_last_error(c.handle).decode() == text

    refused(L.shp_prim_scan(c.handle, d, 1 << 32, d, 0, ctypes.byref(tot), ctypes.byref(mir), None, None), 'bad argument')
    refused(L.shp_prim_scan(c.handle, None, 4, d, 0, ctypes.byref(tot), ctypes.byref(mir), None, None), 'NULL argument')
    refused(L.shp_prim_scan(c.handle, d, 4, None, 0, ctypes.byref(tot), ctypes.byref(mir), None, None), 'NULL argument')
    refused(L.shp_prim_scan(c.handle, d, 4, d, 2, ctypes.byref(tot), ctypes.byref(mir), None, ctypes.byref(nb)),
            'NULL argument')
    refused(L.shp_prim_sort(c.handle, d, None, 1 << 32, 8, 0, None, d, None), 'bad argument')
    refused(L.shp_prim_sort(c.handle, d, None, 4, 33, 0, None, d, None), 'bad argument')
    refused(L.shp_prim_sort(c.handle, None, None, 4, 8, 0, None, d, None), 'NULL argument')
    refused(L.shp_prim_sort(c.handle, d, None, 4, 8, 0, d, None, None), 'NULL argument')
