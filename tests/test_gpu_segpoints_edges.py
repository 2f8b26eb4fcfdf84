"""GPU: the per-segment point lists of csrc/segpoints.h at their run, tile, value and id edges, on one GPU.  Every
case of tests/segpoints_cases.py goes through shp_segpoints_build / _emit by ctypes (and, where a test says so, through
tilingstats.iterSegmentPoints and the resident entry points); the expected offsets, x, y and val always come from
segpoints_helpers.visit_points.  Integer work: numpy.array_equal with dtype, no tolerance.
tests/test_segpoints_cases_host.py proves that each case reaches the edge it is named for."""
import ctypes

import numpy as np
import pytest

import segpoints_cases as C
import segpoints_helpers as H

pytestmark = pytest.mark.gpu

PT = np.dtype([('x', np.uint32), ('y', np.uint32), ('val', np.int64)])


class Lists(object):
    """A context for build / emit and a second one for the resident rasters' copies (any call of a context ends
    the validity of its point lists, so the copies may not go through the first)."""

    def __init__(self):
        from pyshepseg_amd import _lib
        self.lib = _lib
        self.c = _lib.Context()
        self.cc = _lib.Context()
        self.L = self.c._L
        self.bufs = []
        self.spare = np.zeros(4, dtype=np.uint32)

    def close(self):
        self.free()
        self.c.close()
        self.cc.close()

    def free(self):
        for p in self.bufs:
            self.cc.check(self.L.shp_dev_free(self.cc.handle, p))
        self.bufs = []

    def _ptr(self, a):
        return self.lib.ptr(a if a.size else self.spare)        # (an empty raster still has an address to give)

    def resident(self, a):
        p = ctypes.c_void_p()
        self.cc.check(self.L.shp_dev_alloc(self.cc.handle, a.nbytes, ctypes.byref(p)))
        self.bufs.append(p)
        self.cc.check(self.L.shp_dev_upload(self.cc.handle, p, self._ptr(a), a.nbytes))
        return p

    def _args(self, case, dev):
        (seg, band, null, S, tile) = case
        assert seg.dtype == np.uint32 and seg.flags.c_contiguous and band.flags.c_contiguous
        (ps, pb) = (self.resident(seg), self.resident(band)) if dev else (self._ptr(seg), self._ptr(band))
        nullv = np.iinfo(np.int64).min if null is None else int(null)
        return (self.c.handle, ps, pb, self.lib.SHP_DTYPES[band.dtype], seg.shape[0], seg.shape[1], S, nullv)

    def count(self, case, dev=False):
        counts = np.full(case[3] + 1, 0xEEEEEEEE, dtype=np.uint32)
        fn = self.L.shp_segpoints_count_dev if dev else self.L.shp_segpoints_count
        self.c.check(fn(*(self._args(case, dev) + (self.lib.ptr(counts),))))
        return counts

    def build(self, case, dev=False):
        npts = ctypes.c_int64(-1)
        fn = self.L.shp_segpoints_build_dev if dev else self.L.shp_segpoints_build
        self.c.check(fn(*(self._args(case, dev) + (int(case[4]), ctypes.byref(npts)))))
        return npts.value

    def emit_rc(self, lo, hi, cap):
        """(return code, offsets, points, reported count); a guard record behind the cap must keep its filler"""
        offs = np.full(hi - lo + 1, -7, dtype=np.int64)
        pts = np.zeros(cap + 1, dtype=PT)
        pts['val'] = -7
        n = ctypes.c_int64(-1)
        rc = self.L.shp_segpoints_emit(self.c.handle, lo, hi, self.lib.ptr(offs), self.lib.ptr(pts), cap,
                                       ctypes.byref(n))
        assert pts['val'][cap] == -7 and pts['x'][cap] == 0
        return rc, offs, pts[:cap], n.value

    def emit(self, lo, hi, cap):
        (rc, offs, pts, n) = self.emit_rc(lo, hi, cap)
        self.c.check(rc)
        assert n == cap
        return offs, pts


@pytest.fixture(scope='module')
def dev():
    d = Lists()
    yield d
    d.close()


_want = {}


def want(name, case):
    """(offsets of ids 0 .. S + 1, points) by visit_points: computed once per named case, never changed"""
    if name not in _want:
        (seg, band, null, S, tile) = case
        (ids, x, y, val) = H.visit_points(seg, band, null, tile, S)
        offs = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=S + 1))]).astype(np.int64)
        pts = np.zeros(len(ids), dtype=PT)
        (pts['x'], pts['y'], pts['val']) = (x, y, val)
        assert val.dtype == np.int64 and offs[1] == 0 and offs[-1] == len(ids)
        for a in (offs, pts):
            a.flags.writeable = False
        _want[name] = (offs, pts)
    return _want[name]


def same(got, exp):
    return got.dtype == exp.dtype and got.shape == exp.shape and np.array_equal(got, exp)


def check_whole(dev, name, case, resident=False):
    (offs, pts) = want(name, case)
    S = case[3]
    assert dev.build(case, resident) == len(pts)
    (goffs, gpts) = dev.emit(0, S + 1, len(pts))
    assert same(goffs, offs), C_first(goffs, offs)
    for f in ('x', 'y', 'val'):
        assert same(gpts[f], pts[f]), (f, C_first(gpts[f], pts[f]))
    dev.free()


def C_first(got, exp):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(exp)) if got.shape == exp.shape else []
    return 'shapes %s %s' % (got.shape, exp.shape) if got.shape != exp.shape else \
        ('first of %d differences at %d: got %s, expected %s' % (len(bad), bad[0], got[bad[0]], exp[bad[0]])
         if len(bad) else '')


def check_iter(name, case, batch=None):
    """tilingstats.iterSegmentPoints: the batches' ids, offsets and points, concatenated"""
    from pyshepseg_amd import tilingstats as ts
    (seg, band, null, S, tile) = case
    (offs, pts) = want(name, case)
    (ids, got_offs, got) = ([], [np.zeros(1, np.int64)], [])
    total = 0
    for (bid, off, p) in ts.iterSegmentPoints(seg, band, null, tileSize=tile, maxSegId=S, batchPoints=batch):
        assert off[0] == 0 and len(off) == len(bid) + 1 and off[-1] == len(p) and off.dtype == np.int64
        ids.append(np.array(bid))
        got_offs.append(off[1:] + total)
        total += len(p)
        got.append(np.array(p))
    assert np.array_equal(np.concatenate(ids), np.arange(1, S + 1))
    assert same(np.concatenate(got_offs), offs[1:])
    g = np.concatenate(got)
    for f in ('x', 'y', 'val'):
        assert same(g[f], pts[f]), f


# ---- the geometry sweep ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,cols,tile', C.GEOMETRY)
def test_geometry_sweep(dev, rows, cols, tile):
    (case, _p) = C.geometry(rows, cols, tile)
    check_whole(dev, 'geometry-%d-%d-%d' % (rows, cols, tile), case)


@pytest.mark.parametrize('rows,cols', C.SHAPES)
def test_geometry_sweep_iter_and_resident(dev, rows, cols):
    for tile in (2, 64):
        (case, _p) = C.geometry(rows, cols, tile)
        name = 'geometry-%d-%d-%d' % (rows, cols, tile)
        check_iter(name, case, batch=300 if tile == 2 else None)
        check_whole(dev, name, case, resident=True)


def test_geometry_one_id_per_pixel(dev):
    (case, _p) = C.geometry(*C.PER_PIXEL, per_pixel=True)
    check_whole(dev, 'per-pixel', case)
    check_iter('per-pixel', case, batch=1000)


# ---- ballot edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ballot_plain', 'ballot_marks', 'ballot_all_64'])
def test_ballot_edges(dev, name):
    (case, _p) = getattr(C, name)()
    check_whole(dev, name, case)
    check_whole(dev, name, case, resident=True)
    check_iter(name, case)


# ---- expansion ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', [64, 128])
def test_expand_one_id(dev, side):
    (case, _p) = C.expand_one_id(side)
    check_whole(dev, 'one-id-%d' % side, case)
    check_iter('one-id-%d' % side, case)


def _check_range(dev, offs, pts, lo, hi):
    n = int(offs[hi] - offs[lo])
    (goffs, gpts) = dev.emit(lo, hi, n)
    assert same(goffs, offs[lo:hi + 1] - offs[lo]), (lo, hi)
    assert same(gpts, pts[offs[lo]:offs[hi]]), (lo, hi)
    return gpts


@pytest.mark.parametrize('name', ['expand_mixed', 'expand_between', 'ids_gaps'])
def test_expand_ranges(dev, name):
    """every id alone, lo == hi, ranges of two and three ids, ranges without points; the whole list equals the
    concatenation of any partition into ranges"""
    (case, _p) = getattr(C, name)()
    (offs, pts) = want(name, case)
    S = case[3]
    check_whole(dev, name, case)
    assert dev.build(case) == len(pts)
    for lo in range(0, S + 2):
        _check_range(dev, offs, pts, lo, lo)                        # lo == hi: one offset, no point
        for width in (1, 2, 3):
            if lo + width <= S + 1:
                _check_range(dev, offs, pts, lo, lo + width)
    rng = np.random.RandomState(3)
    for _k in range(3):
        cuts = np.unique(np.r_[0, rng.randint(0, S + 2, size=3), S + 1])
        parts = [_check_range(dev, offs, pts, int(a), int(b)) for (a, b) in zip(cuts, cuts[1:])]
        assert same(np.concatenate(parts), np.array(pts))
    check_iter(name, case, batch=2000)


def test_emit_cap(dev):
    """cap equal to the count passes; one below is refused with the count reported; a correct emit still passes"""
    (case, _p) = C.expand_mixed()
    (offs, pts) = want('expand_mixed', case)
    assert dev.build(case) == len(pts)
    (lo, hi) = (3, 6)
    n = int(offs[hi] - offs[lo])
    _check_range(dev, offs, pts, lo, hi)
    (rc, _o, got, reported) = dev.emit_rc(lo, hi, n - 1)
    assert rc == -3 and reported == n and (got['val'] == -7).all()          # SHP_ERR_ARG
    msg = dev.L.shp_last_error(dev.c.handle).decode()
    assert 'hold %d points' % n in msg and 'the output %d' % (n - 1) in msg
    with pytest.raises(dev.lib.ShepsegHipError, match='hold %d points' % n):
        dev.c.check(dev.emit_rc(lo, hi, 0)[0])
    _check_range(dev, offs, pts, lo, hi)
    _check_range(dev, offs, pts, 0, case[3] + 1)


# ---- ids ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ids_above_max', 'ids_single', 'ids_gaps'])
def test_id_edges(dev, name):
    (case, _p) = getattr(C, name)()
    check_whole(dev, name, case)
    check_whole(dev, name, case, resident=True)
    check_iter(name, case)


def test_ids_sparse_up_to_2_pow_20(dev):
    """S = 2^20 with five ids present: the offsets of all S + 1 ids (and the end)"""
    (case, p) = C.ids_sparse_large()
    (offs, pts) = want('ids_sparse_large', case)
    assert len(offs) == (1 << 20) + 2
    check_whole(dev, 'ids_sparse_large', case)
    assert dev.build(case) == len(pts)
    for i in p['present'].tolist():
        _check_range(dev, offs, pts, i, i + 1)
    _check_range(dev, offs, pts, 257, 70000)
    check_iter('ids_sparse_large', case)


@pytest.mark.parametrize('kind', ['zero', 'nodata', 'norows', 'nocols'])
def test_rasters_without_a_point(dev, kind):
    (case, _p) = C.empty(kind)
    S = case[3]
    for resident in (False, True):
        assert np.array_equal(dev.count(case, resident), np.zeros(S + 1, np.uint32))
        assert dev.build(case, resident) == 0
        (rc, offs, _pts, n) = dev.emit_rc(0, S + 1, 0)
        assert rc == 0 and n == 0 and same(offs, np.zeros(S + 2, np.int64))
        (rc, offs, _pts, n) = dev.emit_rc(2, 3, 5)
        assert rc == 0 and n == 0 and same(offs, np.zeros(2, np.int64))
        dev.free()
    check_iter('empty-' + kind, case)


# ---- values ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', C.DTYPES)
def test_values_at_every_limit(dev, dtype):
    """val comes back as the exact int64; nodata at either limit of the type; outside its range nothing is nodata"""
    for null in C.value_nulls(dtype):
        (case, p) = C.values(dtype, null)
        name = 'values-%s-%d' % (np.dtype(dtype).name, null)
        (offs, pts) = want(name, case)
        check_whole(dev, name, case)
        check_iter(name, case)
        assert set(pts['val'].tolist()) == set(p['values'].tolist()) - {null}
    check_whole(dev, name, case, resident=True)


# ---- host and resident entry points ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ballot_marks', 'expand_mixed', 'values_int32'])
def test_host_and_resident_agree(dev, name):
    (case, _p) = C.values(np.int32, -2 ** 31) if name == 'values_int32' else getattr(C, name)()
    (offs, pts) = want('agree-' + name, case)
    S = case[3]
    lists = []
    for resident in (False, True):
        counts = dev.count(case, resident)
        assert same(counts, np.diff(offs).astype(np.uint32))
        n = dev.build(case, resident)
        assert n == int(counts.sum(dtype=np.int64))
        lists.append(dev.emit(0, S + 1, n))
        dev.free()
    assert same(lists[0][0], lists[1][0]) and same(lists[0][1], lists[1][1])
    assert same(lists[0][0], offs) and same(lists[0][1], np.array(pts))
