"""GPU: the subset recode (csrc/subset.h) at its tile, key-width, id-range and shard edges, on hand-built inputs
(tests/subset_cases.py) against the plain model there, which tests/test_subset_cases_host.py ties to the oracle and
the reference's goldens.  Integer work: numpy.array_equal throughout.

What each group is aimed at:
 A  subset_key -- th and tw clipped separately in the last tile row / column, a tile larger than the window in one
    or both directions, tile 1 and 1 << 30 -- on labels that make the output every pixel's key + 1, and the keys
    themselves as the local step of one shard reports them (the output is their order only); subset_id's
    tlx / tly / img_cols; k_subset_first's left / upper neighbour tests under masks that move an id's first pixel.
 B  subset_number's key width bits_for(n_win - 1) where the sort's pass count changes, and m across the sort's and
    the scan's blocks.
 C  the scan and k_subset_list over max_seg_id + 1 ids at the scan's sub-block / block edges and the 256-thread
    grid edge, max_seg_id far above the ids present, m = 1; how much of orig_out / hist_out is written.
 D  subset_check and run_subset_recode's two data-dependent refusals, and the context after a refusal.
 E  run_dsubset_local / run_dsubset_merge: the slice geometry (base_row, r0, nr), `r > g.r0`, k_subset_scatter's
    slot padding and id filter, the zeroing of d_hist up to cap.

The output of every call lies between guard words that must keep their filler; orig_out / hist_out beyond the
m + 1 rows written keep theirs."""
import ctypes

import numpy as np
import pytest

import prim_cases as pc
import subset_cases as sc

pytestmark = pytest.mark.gpu

SHP_ERR_ARG = -3
FILL = pc.FILL_WORD
UNSET = 0x12345678


class Rig(object):
    """the calling thread's context, its named device buffers (prim_cases.Dev) and the entry points of the recode"""

    def __init__(self):
        self.dev = pc.Dev()
        (self.c, self.L) = (self.dev.c, self.dev.L)

    def close(self):
        self.dev.close()

    def upload_bytes(self, name, a):
        a = np.ascontiguousarray(a, dtype=np.uint8).ravel()
        words = np.zeros(-(-a.size // 4) * 4, dtype=np.uint8)
        words[:a.size] = a
        return self.dev.upload(name, words.view(np.uint32))

    def message(self, rc):
        return (self.L.shp_last_error(self.c.handle) or b'').decode() if rc else ''

    def recode_dev(self, seg, win, mask, T, max_id, cap):
        "shp_subset_recode_dev -> Result"
        (tlx, tly, xs, ys) = win
        n = max(xs, 0) * max(ys, 0)
        d_seg = self.dev.upload('seg', seg.ravel())
        d_mask = self.upload_bytes('mask', mask) if mask is not None else None
        d_out = self.dev.guarded('out', n)
        r = Result(n, cap)
        r.rc = self.L.shp_subset_recode_dev(self.c.handle, d_seg, seg.shape[0], seg.shape[1], tlx, tly, xs, ys, d_mask,
                                            T, max_id, d_out, pc_ptr(r.orig), pc_ptr(r.hist), cap, ctypes.byref(r.nn))
        r.msg = self.message(r.rc)
        (r.out, r.clean) = self.dev.fetch('out', n)
        return r

    def recode_host(self, seg, win, mask, T, max_id, cap):
        "shp_subset_recode -> Result"
        (tlx, tly, xs, ys) = win
        n = max(xs, 0) * max(ys, 0)
        room = np.full(n + 2 * pc.GUARD, FILL, dtype=np.uint32)
        r = Result(n, cap)
        r.out = room[pc.GUARD:pc.GUARD + n]
        mask = np.ascontiguousarray(mask) if mask is not None else None
        r.rc = self.L.shp_subset_recode(self.c.handle, pc_ptr(seg), seg.shape[0], seg.shape[1], tlx, tly, xs, ys,
                                        pc_ptr(mask) if mask is not None else None, T, max_id, pc_ptr(r.out),
                                        pc_ptr(r.orig), pc_ptr(r.hist), cap, ctypes.byref(r.nn))
        r.msg = self.message(r.rc)
        r.clean = bool((room[:pc.GUARD] == FILL).all() and (room[pc.GUARD + n:] == FILL).all())
        return r

    ENTRIES = ('recode_dev', 'recode_host')


def pc_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Result(object):
    def __init__(self, n, cap):
        self.orig = np.full(max(cap, 1), FILL, dtype=np.uint32)
        self.hist = np.full(max(cap, 1), FILL, dtype=np.uint32)
        self.nn = ctypes.c_uint32(UNSET)
        (self.rc, self.msg, self.out, self.clean) = (None, '', None, None)


@pytest.fixture(scope='module')
def rig():
    r = Rig()
    yield r
    r.close()


def check(r, want, tag):
    "a Result against (out, orig, hist) of the model"
    (out, orig, hist) = want
    m = len(orig) - 1
    assert r.rc == 0, '%s: error %d: %s' % (tag, r.rc, r.msg)
    assert r.nn.value == m, '%s: %d new ids, expected %d' % (tag, r.nn.value, m)
    assert r.clean, tag + ': words around the output window were written'
    diff = pc.first_diff(r.out, out.ravel())
    assert not diff, '%s: out: %s' % (tag, diff)
    diff = pc.first_diff(r.orig[:m + 1], orig)
    assert not diff, '%s: orig: %s' % (tag, diff)
    diff = pc.first_diff(r.hist[:m + 1], hist)
    assert not diff, '%s: hist: %s' % (tag, diff)
    assert (r.orig[m + 1:] == FILL).all() and (r.hist[m + 1:] == FILL).all(), tag + ': rows beyond m + 1 were written'


def check_entries(rig, case, extra=5, entries=Rig.ENTRIES):
    want = case.want()
    cap = len(want[1]) + extra
    for entry in entries:
        r = getattr(rig, entry)(case.seg, case.win, case.mask, case.T, case.max_seg_id, cap)
        check(r, want, '%s %s' % (case.name, entry))


def check_wrapper(case):
    "subset.subsetImage, which copies the window to (0, 0) and passes its largest id"
    from pyshepseg_amd import subset
    (out, orig, hist) = case.want()
    r = subset.subsetImage(case.seg, None, case.tlx, case.tly, case.xs, case.ys, maskImage=case.mask, tileSize=case.T)
    diff = pc.first_diff(r.segimg, out)
    assert not diff, '%s subsetImage: out: %s' % (case.name, diff)
    assert np.array_equal(r.origSegIds, orig) and np.array_equal(r.hist, hist), case.name


# ---- A: every pixel's key ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sc.PERM_CASES, ids=lambda c: c.name)
def test_every_pixels_key(rig, case):
    (out, orig, hist) = case.want()
    assert np.array_equal(out, sc.visit_keys(case.ys, case.xs, case.T) + 1) and (hist[1:] == 1).all()
    check_entries(rig, case)
    check_wrapper(case)
    # the keys themselves, as one shard holding the whole raster reports them: ids ascending is raster order here
    d_seg = rig.dev.upload('seg', case.seg.ravel())
    (p, n) = local(rig, case, d_seg, 0, case.seg.shape[0], None)
    assert n == case.xs * case.ys
    got = np.empty(2 * n, dtype=np.uint32)
    rig.c.check(rig.L.shp_dev_download(rig.c.handle, pc_ptr(got), p, got.nbytes))
    assert np.array_equal(got[n:], np.arange(1, n + 1))
    diff = pc.first_diff(got[:n], sc.visit_keys(case.ys, case.xs, case.T).ravel())
    assert not diff, '%s: keys: %s' % (case.name, diff)


@pytest.mark.parametrize('case', sc.BLOCKY_CASES, ids=lambda c: c.name)
def test_blocky_labels(rig, case):
    check_entries(rig, case)
    check_wrapper(case)


# ---- B: key width ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sc.WIDTH_CASES, ids=lambda c: c.name)
def test_key_width(rig, case):
    check_entries(rig, case, extra=3, entries=('recode_dev',))
    check_wrapper(case)


# ---- C: id range -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sc.RANGE_CASES + sc.SINGLE_ID_CASES, ids=lambda c: c.name)
def test_id_range(rig, case):
    check_entries(rig, case, extra=7)


@pytest.mark.parametrize('case', [c for c in sc.RANGE_CASES if c.max_seg_id == sc.SCAN_ITEMS + 1],
                         ids=lambda c: c.name)
def test_window_inside_a_wider_raster_equals_the_wrapper(rig, case):
    """tlx, tly > 0 and img_cols > xs through both entry points give what subset.subsetImage gives"""
    from pyshepseg_amd import subset
    assert case.tlx > 0 and case.tly > 0 and case.seg.shape[1] > case.xs
    w = subset.subsetImage(case.seg, None, *case.win, maskImage=case.mask, tileSize=case.T)
    for entry in Rig.ENTRIES:
        r = getattr(rig, entry)(case.seg, case.win, case.mask, case.T, case.max_seg_id, len(w.origSegIds))
        check(r, (w.segimg, w.origSegIds, w.hist), '%s %s' % (case.name, entry))


# ---- D: errors, and the context afterwards -------------------------------------------------------------------------------
BASE = sc.RANGE_CASES[0]                # unmasked, max_seg_id the true maximum SCAN_ITEMS + 1
BASE_MASKED = [c for c in sc.RANGE_CASES if c.mask is not None][0]


def refused(rig, entry, match, seg, win, mask, T, max_id, cap):
    r = getattr(rig, entry)(seg, win, mask, T, max_id, cap)
    tag = '%s (%s)' % (match, entry)
    assert r.rc == SHP_ERR_ARG, '%s: returned %d %s' % (tag, r.rc, r.msg)
    assert match in r.msg, '%s: message %r' % (tag, r.msg)
    assert r.clean, tag
    # the next valid call on the same context is right
    check(getattr(rig, entry)(BASE.seg, BASE.win, None, BASE.T, BASE.max_seg_id, len(BASE.want()[1])), BASE.want(),
          'after ' + tag)
    return r


@pytest.mark.parametrize('entry', Rig.ENTRIES)
def test_id_above_max_seg_id(rig, entry):
    m1 = len(BASE.want()[1])
    # inside the window: refused (the largest id present is SCAN_ITEMS + 1)
    r = refused(rig, entry, 'segment id above max_seg_id (%d)' % sc.SCAN_ITEMS, BASE.seg, BASE.win, None, BASE.T,
                sc.SCAN_ITEMS, m1)
    assert r.nn.value == 0
    # outside the window: not looked at
    seg = BASE.seg.copy()
    seg[0, 0] = seg[BASE.tly - 1, BASE.tlx + 4] = seg[BASE.tly + 4, BASE.tlx - 1] = 1 << 24
    check(getattr(rig, entry)(seg, BASE.win, None, BASE.T, BASE.max_seg_id, m1), BASE.want(), 'outside the window')
    # under a zero mask pixel: not looked at either
    c = BASE_MASKED
    seg = c.seg.copy()
    seg[c.tly:, c.tlx:][c.mask == 0] = 1 << 24
    check(getattr(rig, entry)(seg, c.win, c.mask, c.T, c.max_seg_id, len(c.want()[1])), c.want(), 'under the mask')


@pytest.mark.parametrize('entry', Rig.ENTRIES)
def test_cap(rig, entry):
    m = len(BASE.want()[1]) - 1
    refused(rig, entry, 'subset holds %d segments, output arrays hold %d rows' % (m, m), BASE.seg, BASE.win, None,
            BASE.T, BASE.max_seg_id, m)
    check(getattr(rig, entry)(BASE.seg, BASE.win, None, BASE.T, BASE.max_seg_id, m + 1), BASE.want(), 'cap = m + 1')


@pytest.mark.parametrize('entry', Rig.ENTRIES)
def test_argument_refusals(rig, entry):
    (tlx, tly, xs, ys) = BASE.win
    cap = len(BASE.want()[1])
    assert BASE.seg.shape == (tly + ys, tlx + xs)
    for win in ((tlx, tly, xs + 1, ys), (tlx, tly, xs, ys + 1), (tlx + 1, tly, xs, ys), (tlx, tly + 1, xs, ys)):
        refused(rig, entry, 'Requested subset is not within input image', BASE.seg, win, None, BASE.T,
                BASE.max_seg_id, cap)
    refused(rig, entry, 'bad argument', BASE.seg, BASE.win, None, 0, BASE.max_seg_id, cap)
    # the largest label there is: max_seg_id + 1 ids do not count in 32 bits
    tiny = np.array([[1, 2], [2, sc.M32]], dtype=np.uint32)
    refused(rig, entry, 'max_seg_id too large', tiny, (0, 0, 2, 2), None, 1024, sc.M32, 5)
    # ... whether or not the window holds it, and before an empty window returns
    refused(rig, entry, 'max_seg_id too large', tiny, (0, 0, 2, 1), None, 1024, sc.M32, 5)
    refused(rig, entry, 'max_seg_id too large', tiny, (0, 0, 0, 0), None, 1024, sc.M32, 5)


@pytest.mark.parametrize('entry', Rig.ENTRIES)
def test_empty_window(rig, entry):
    for win in ((BASE.tlx, BASE.tly, 0, 5), (BASE.tlx, BASE.tly, 5, 0), (0, 0, 0, 0)):
        r = getattr(rig, entry)(BASE.seg, win, None, BASE.T, BASE.max_seg_id, 4)
        assert r.rc == 0 and r.nn.value == 0 and r.clean, (win, r.rc, r.msg)
        assert (r.orig == FILL).all() and (r.hist == FILL).all()


def test_wrapper_refuses_the_largest_label():
    from pyshepseg_amd import subset
    tiny = np.array([[1, 2], [2, sc.M32]], dtype=np.uint32)
    with pytest.raises(subset.PyShepSegSubsetError, match='too large'):
        subset.subsetImage(tiny, None, 0, 0, 2, 2)
    r = subset.subsetImage(tiny, None, 0, 0, 2, 2, maskImage=np.array([[1, 1], [1, 0]], np.uint8), tileSize=1)
    assert r.segimg.tolist() == [[1, 2], [2, 0]] and r.origSegIds.tolist() == [0, 1, 2] and r.hist.tolist() == [0, 1, 2]


# ---- E: the sharded kernels, played in one process -------------------------------------------------------------------------
def local(rig, case, d_seg, lo, hi, d_mask):
    """shp_dsubset_local_dev of the shard of image rows [lo, hi) of case.seg (at d_seg; d_mask: the whole window's
    mask or None) -> (device address of the n keys and n ids in the context's workspace, n).  A shard that holds
    no window row passes no labels"""
    (tlx, tly, xs, ys) = case.win
    (a, b) = sc.held_rows(lo, hi, tly, ys)
    ncols = case.seg.shape[1]
    (p, n, bad) = (ctypes.c_void_p(), ctypes.c_int64(-1), ctypes.c_int(-1))
    rig.c.check(rig.L.shp_dsubset_local_dev(
        rig.c.handle, d_seg + lo * ncols * 4 if b > a else None, hi - lo, ncols, lo, case.max_seg_id, tlx, tly, xs, ys,
        case.T, d_mask + a * xs if d_mask is not None and b > a else None, ctypes.byref(p), ctypes.byref(n),
        ctypes.byref(bad)))
    assert bad.value == 0 and n.value >= 0
    return p.value, n.value


def merge(rig, d_pairs, slot, counts, d_seg, lo, hi, ncols, max_id, win, T, d_mask, held, cap):
    """shp_dsubset_merge_dev of the shard of image rows [lo, hi) holding window rows `held` -> (rows, hist words,
    orig, m)"""
    (tlx, tly, xs, ys) = win
    (a, b) = held
    n = (b - a) * xs
    d_out = rig.dev.guarded('rows', n) if n else None
    d_hist = rig.dev.guarded('hist', cap)
    orig = np.full(cap, FILL, dtype=np.uint32)
    nn = ctypes.c_uint32(UNSET)
    rig.c.check(rig.L.shp_dsubset_merge_dev(rig.c.handle, d_pairs, slot, len(counts), pc_ptr(counts),
                                            d_seg if n else None, hi - lo, ncols, lo, max_id, tlx, tly, xs, ys, T,
                                            d_mask if n else None, d_out, d_hist, pc_ptr(orig), cap, ctypes.byref(nn)))
    (hist, clean) = rig.dev.fetch('hist', cap)
    assert clean, 'words around d_hist were written'
    rows = np.zeros(0, dtype=np.uint32)
    if n:
        (rows, clean) = rig.dev.fetch('rows', n)
        assert clean, 'words around the recoded rows were written'
    return rows.copy(), hist.copy(), orig, nn.value


@pytest.mark.parametrize('T', sc.SHARD_TILES)
@pytest.mark.parametrize('layout', sc.SHARD_LAYOUTS)
def test_shards(rig, layout, T):
    cuts = sc.shard_cuts(layout, T)
    shards = list(zip(cuts, cuts[1:]))
    world = len(shards)
    for masked in (False, True):
        case = sc.SHARD_CASES[(T, masked)]
        (out, orig, hist) = case.want()
        m = len(orig) - 1
        (tlx, tly, xs, ys) = case.win
        ncols = case.seg.shape[1]
        d_seg = rig.dev.upload('seg', case.seg.ravel())
        d_mask = rig.upload_bytes('mask', case.mask) if masked else None
        held = [sc.held_rows(lo, hi, tly, ys) for (lo, hi) in shards]
        # local: every shard's pairs, copied into its slot before the next call reuses the workspace
        slot = m                                        # no shard can report more
        d_all = rig.dev.guarded('gathered', world * 2 * slot)
        counts = np.zeros(world, dtype=np.uint32)
        for r, ((lo, hi), (a, b)) in enumerate(zip(shards, held)):
            (p, n) = local(rig, case, d_seg, lo, hi, d_mask)
            assert n <= slot
            counts[r] = n
            if n:
                rig.c.check(rig.L.shp_dev_copy(rig.c.handle, d_all + r * 2 * slot * 4, p, n * 8))
        (words, clean) = rig.dev.fetch('gathered', world * 2 * slot)
        assert clean
        for r, (a, b) in enumerate(held):
            (keys, ids) = sc.shard_first(case.seg, *case.args, rows=(a, b))
            tag = '%s %s shard %d (window rows %d..%d): ' % (case.name, layout, r, a, b)
            assert counts[r] == len(ids), tag + '%d pairs, expected %d' % (counts[r], len(ids))
            got = words[r * 2 * slot:][:2 * len(ids)]
            assert np.array_equal(got[len(ids):], ids), tag + 'ids'
            diff = pc.first_diff(got[:len(ids)], keys)
            assert not diff, tag + 'keys: ' + diff
        # merge, on every shard
        cap = m + 1 + 37
        stacked = []
        hsum = np.zeros(cap, dtype=np.int64)
        for r, ((lo, hi), (a, b)) in enumerate(zip(shards, held)):
            (rows, h, o, mm) = merge(rig, d_all, slot, counts, d_seg + lo * ncols * 4, lo, hi, ncols, case.max_seg_id,
                                     case.win, T, d_mask + a * xs if masked else None, (a, b), cap)
            tag = '%s %s shard %d: ' % (case.name, layout, r)
            assert mm == m, tag + '%d new ids, expected %d' % (mm, m)
            assert np.array_equal(o[:m + 1], orig) and (o[m + 1:] == FILL).all(), tag + 'orig'
            assert (h[m + 1:] == 0).all(), tag + 'd_hist is not zero from m + 1 up to cap'
            stacked.append(rows)
            hsum += h
        diff = pc.first_diff(np.concatenate(stacked), out.ravel())
        assert not diff, '%s %s: stacked rows: %s' % (case.name, layout, diff)
        assert np.array_equal(hsum[:m + 1], hist.astype(np.int64)), '%s %s: summed hist' % (case.name, layout)


def test_hand_built_pairs(rig):
    """only the numbering: no shard holds a row.  Slot padding that reads as a valid pair, a rank without pairs, an
    id whose minimum is on the last rank, ids 0 and above max_seg_id, keys in no order"""
    (words, counts) = sc.gathered_pairs()
    d_pairs = rig.dev.upload('pairs', words)
    (xs, ys) = sc.PAIRS_WIN
    cap = 16
    (rows, hist, orig, m) = merge(rig, d_pairs, sc.PAIRS_SLOT, counts, None, 0, 0, xs, sc.PAIRS_MAX_ID, (0, 0, xs, ys),
                                  8, None, (0, 0), cap)
    assert m == len(sc.PAIRS_ORIG) - 1
    assert orig[:m + 1].tolist() == list(sc.PAIRS_ORIG) and (orig[m + 1:] == FILL).all()
    assert (hist == 0).all() and rows.size == 0
