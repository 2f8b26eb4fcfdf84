"""GPU: the cross-tile stitch on the generated label tilings of tests/stitch_cases.py, in its three forms,
against the numpy model of the reference's stitch (array_equal throughout):
  chain     shp_stitch_prepare_dev per tile + the tiled driver's chain step (_StitchBuffers.step): mosaic,
            maxSegId, histogram, and per tile the meta block (flags, bounding-box corner, LUT), the counted
            crossing pixels and the recoded strips handed on
  one_call  shp_stitch_tile_dev, every tile recoded in place, the neighbours' strips read from their tiles
  parallel  the chain step on provisional bases + shp_stitch_counts_dev + shp_renumber_dev"""
import ctypes

import numpy as np
import pytest

import stitch_cases as sc

pytestmark = pytest.mark.gpu

UNKNOWN = 0xFFFFFFFF
RANDOM_PARTS = ['random:%d' % i for i in range(4)]     # the 20 seeds, five per test
GROUPS = [g for g in sc.GROUPS if g != 'random'] + RANDOM_PARTS


@pytest.fixture(scope='module', autouse=True)
def _device_cache():
    yield
    from pyshepseg_amd import tiling
    tiling.clearDeviceCache()                           # the blocks the runs handed back


def _cases(name):
    if name.startswith('random:'):
        k = int(name.split(':')[1])
        return sc.group('random')[5 * k:5 * k + 5]
    return sc.group(name)


def _down(c, dptr, n):
    a = np.zeros(max(int(n), 1), dtype=np.uint32)
    c.check(c._L.shp_dev_download(c.handle, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(dptr), 4 * a.size))
    return a[:int(n)]


def _up(c, dptr, a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    c.check(c._L.shp_dev_upload(c.handle, ctypes.c_void_p(dptr), a.ctypes.data_as(ctypes.c_void_p), 4 * a.size))


class _Run(object):
    """A case's tiles in the device blocks of the tiled driver (tiling._StitchBuffers), prepared."""

    def __init__(self, case, simple=False, known_px=True):
        from pyshepseg_amd import _lib, tiling
        (self.case, self.simple, self.tiling) = (case, simple, tiling)
        self.c = c = _lib.ctx()
        self.L = c._L
        ti = tiling.TileInfo()
        for ((col, row), (x, y, xs, ys)) in case.geom.items():
            ti.addTile(x, y, xs, ys, col, row)
        (ti.ncols, ti.nrows) = (case.ntc, case.ntr)
        self.ti = ti
        (self.jobs, self.total) = tiling.makeTileJobs(ti)
        assert [(j.col, j.row) for j in self.jobs] == case.order()
        self.jobmap = {(j.col, j.row): j for j in self.jobs}
        self.extra = []
        self.ok = False
        self.bufs = tiling._StitchBuffers(c, ti, self.jobs, self.total, 0, case.nr, case.nc, case.overlap, zeroOut=True)
        try:
            self._prepare(case, simple, known_px)
        except Exception:
            self.close()
            raise

    def _prepare(self, case, simple, known_px):
        (c, ti, tiling) = (self.c, self.ti, self.tiling)
        self.cross = {}
        for j in self.jobs:
            t = case.tiles[(j.col, j.row)]
            assert t.shape == (j.ysize, j.xsize)
            _up(c, self.bufs.d_tiles.value + 4 * j.offset, t)
            j.maxLocal = int(t.max())
        self.wins = {(j.col, j.row): tiling.trimmedWindow(ti, j.col, j.row, j.xpos, j.ypos, j.xsize, j.ysize,
                                                          case.overlap) for j in self.jobs}
        for j in self.jobs:                             # what a worker does after segmenting the tile
            assert self.wins[(j.col, j.row)] == case.window(j.col, j.row)
            (top, bottom, left, right, _x, _y) = self.wins[(j.col, j.row)]
            j.meta = self.bufs.arena.alloc(j.maxLocal + 1, c)
            cross = (ctypes.c_uint32 * 2)(0, 0)
            c.check(self.L.shp_stitch_prepare_dev(
                c.handle, ctypes.c_void_p(self.bufs.d_tiles.value + 4 * j.offset), j.ysize, j.xsize, case.overlap,
                int(j.row > 0 and not simple), int(j.col > 0 and not simple), j.maxLocal, top, bottom, left, right,
                ctypes.c_void_p(j.meta), cross))
            self.cross[(j.col, j.row)] = [int(cross[0]), int(cross[1])]
            j.crossPx = (int(cross[0]), int(cross[1])) if known_px else (UNKNOWN, UNKNOWN)

    def alloc(self, nbytes):
        d = self.tiling._devAlloc(self.c, nbytes)
        self.extra.append((d, max(int(nbytes), 16)))
        return d

    def neighbours(self, j):
        top = self.bufs.bottomStrip(self.jobmap[(j.col, j.row - 1)]) if (j.row > 0 and not self.simple) else None
        left = self.bufs.rightStrip(self.jobmap[(j.col - 1, j.row)]) if (j.col > 0 and not self.simple) else None
        return (top, left)

    def chain(self, bases=None):
        for (t, j) in enumerate(self.jobs):
            (top, left) = self.neighbours(j)
            self.bufs.step(j, top, left, self.wins[(j.col, j.row)], self.simple,
                           scalar=None if bases is None else bases + 4 * t)
        self.sync()

    def sync(self):
        self.c.check(self.L.shp_sync(self.c.handle))

    def mosaic(self, d_out=None):
        d = self.bufs.d_out.value if d_out is None else d_out
        return _down(self.c, d, self.case.nr * self.case.nc).reshape(self.case.nr, self.case.nc)

    def hist(self, max_seg, d_out=None):
        h = np.zeros(max_seg + 1, dtype=np.uint32)
        d = self.bufs.d_out if d_out is None else ctypes.c_void_p(d_out)
        self.c.check(self.L.shp_histogram_dev(self.c.handle, d, self.case.nr * self.case.nc, self.case.nc, max_seg,
                                              h.ctypes.data_as(ctypes.c_void_p)))
        return h

    def close(self):
        for (d, n) in self.extra:
            if self.ok:
                self.tiling._devRelease(self.c, d, n)
            else:
                self.L.shp_dev_free(self.c.handle, d)
        self.extra = []
        if self.ok:
            self.bufs.release()
        else:
            self.bufs.free()


def _check_outputs(run, m, max_seg, d_out=None):
    assert max_seg == m.maxSegId, run.case.name
    assert np.array_equal(run.mosaic(d_out), m.mosaic), run.case.name
    # (only now: the histogram call trusts that no id of the raster is above the maximum it is given)
    assert np.array_equal(run.hist(m.maxSegId, d_out), m.hist), run.case.name


def _run_chain(case, simple=False, known_px=True):
    m = sc.model_stitch(case, simple=simple)
    run = _Run(case, simple=simple, known_px=known_px)
    try:
        run.chain()
        strips = _down(run.c, run.bufs.d_strips.value, run.bufs.nbStrips // 4)
        o = case.overlap
        for j in run.jobs:
            key = (j.col, j.row)
            res = m.tiles[key]
            nseg = j.maxLocal + 1
            meta = _down(run.c, j.meta, 4 * nseg).reshape(4, nseg)
            (flags, segtop, segleft, lut) = meta
            assert run.cross[key] == list(res.cross_px), (case.name, key)
            assert np.array_equal((flags[1:] & 1) != 0, res.cross_top[1:]), (case.name, key)
            assert np.array_equal((flags[1:] & 2) != 0, res.cross_left[1:]), (case.name, key)
            assert np.array_equal((flags[1:] & 4) != 0, res.in_trim[1:]), (case.name, key)
            assert not (flags & ~np.uint32(7)).any() and flags[0] == 0
            assert np.array_equal(segtop[1:], res.segtop[1:]), (case.name, key)
            assert np.array_equal(segleft[1:], res.segleft[1:]), (case.name, key)
            assert np.array_equal(lut, res.lut), (case.name, key)
            if res.right is not None:
                w = min(o, j.xsize)
                got = strips[j.rightOff:j.rightOff + j.ysize * w].reshape(j.ysize, w)
                assert np.array_equal(got, res.right), (case.name, key)
            if res.bottom is not None:
                h = min(o, j.ysize)
                got = strips[j.bottomOff:j.bottomOff + h * j.xsize].reshape(h, j.xsize)
                assert np.array_equal(got, res.bottom), (case.name, key)
        _check_outputs(run, m, int(_down(run.c, run.bufs.d_scal.value, 1)[0]))
        run.ok = True
    finally:
        run.close()


@pytest.mark.parametrize('name', GROUPS)
def test_chain(name):
    for case in _cases(name):
        _run_chain(case)


@pytest.mark.parametrize('name', ['ties', 'dense_pairs'] + RANDOM_PARTS)
def test_chain_unknown_cross_px(name):
    """the pair table sized by the whole strip (0xFFFFFFFF = the crossing pixels were not counted)"""
    for case in _cases(name):
        _run_chain(case, known_px=False)


@pytest.mark.parametrize('name', ['ties/3x3', 'random/05'])
def test_chain_simple(name):
    _run_chain(sc.case(name), simple=True)


@pytest.mark.parametrize('name', GROUPS)
def test_one_call(name):
    """shp_stitch_tile_dev in tile order on a private copy of the tile block: the strips of the tiles above and
    to the left are read where those tiles were recoded, with the row pitch of those tiles"""
    for case in _cases(name):
        m = sc.model_stitch(case)
        run = _Run(case)
        try:
            c = run.c
            d_tiles = run.alloc(4 * run.total)
            c.check(run.L.shp_dev_copy(c.handle, d_tiles, run.bufs.d_tiles, 4 * run.total))
            d_out = run.alloc(4 * case.nr * case.nc)
            c.check(run.L.shp_dev_memset(c.handle, d_out, 0, 4 * case.nr * case.nc))
            d_max = run.alloc(256)
            c.check(run.L.shp_dev_memset(c.handle, d_max, 0, 256))
            o = case.overlap
            for j in run.jobs:
                (top, bottom, left, right, xout, yout) = run.wins[(j.col, j.row)]
                (tb, tp, lb, lp) = (None, 0, None, 0)
                if j.row > 0:
                    a = run.jobmap[(j.col, j.row - 1)]
                    tb = ctypes.c_void_p(d_tiles.value + 4 * (a.offset + (a.ysize - min(o, a.ysize)) * a.xsize))
                    tp = a.xsize
                if j.col > 0:
                    a = run.jobmap[(j.col - 1, j.row)]
                    lb = ctypes.c_void_p(d_tiles.value + 4 * (a.offset + a.xsize - min(o, a.xsize)))
                    lp = a.xsize
                c.check(run.L.shp_stitch_tile_dev(
                    c.handle, ctypes.c_void_p(d_tiles.value + 4 * j.offset), j.ysize, j.xsize, o, tb, tp, lb, lp,
                    j.maxLocal, 0, d_max, top, bottom, left, right, d_out, case.nc, xout, yout))
            run.sync()
            max_seg = int(_down(c, d_max.value, 1)[0])
            _check_outputs(run, m, max_seg, d_out.value)
            tiles = _down(c, d_tiles.value, run.total)
            for j in run.jobs:
                got = tiles[j.offset:j.offset + j.ysize * j.xsize].reshape(j.ysize, j.xsize)
                assert np.array_equal(got, m.tiles[(j.col, j.row)].recoded), (case.name, j.col, j.row)
            run.ok = True
        finally:
            run.close()


@pytest.mark.parametrize('name', GROUPS)
def test_parallel(name):
    """every tile numbers its new ids from a provisional base of its own; the counts K (new ids) and R (the
    largest of them in the trimmed window) are the model's, and where they agree everywhere the renumbered
    raster is the sequential mosaic"""
    for case in _cases(name):
        m = sc.model_stitch(case)
        run = _Run(case)
        try:
            c = run.c
            nt = len(run.jobs)
            stride = 0xFFFFFFFF // nt
            d_bases = run.alloc(4 * 3 * nt)
            c.check(run.L.shp_dev_memset(c.handle, d_bases, 0, 4 * 3 * nt))
            _up(c, d_bases.value, (np.arange(nt, dtype=np.uint64) * stride).astype(np.uint32))
            for (t, j) in enumerate(run.jobs):
                (top, left) = run.neighbours(j)
                run.bufs.step(j, top, left, run.wins[(j.col, j.row)], False, scalar=d_bases.value + 4 * t)
                c.check(run.L.shp_stitch_counts_dev(c.handle, ctypes.c_void_p(j.meta), j.maxLocal, t * stride,
                                                    ctypes.c_void_p(d_bases.value + 4 * (nt + 2 * t))))
            run.sync()
            counts = _down(c, d_bases.value + 4 * nt, 2 * nt).reshape(nt, 2)
            want = np.array([[m.tiles[k].K, m.tiles[k].R] for k in case.order()], dtype=np.uint32)
            assert np.array_equal(counts, want), case.name
            differ = [k for k in case.order() if m.tiles[k].K != m.tiles[k].R]
            assert differ == m.census['k_ne_r_tiles']
            if case.group == 'outside_owner':
                assert [case.order()[t] for t in range(nt) if counts[t, 0] != counts[t, 1]] == [(0, 0)]
            if not differ:
                base = np.concatenate([[0], np.cumsum(counts[:, 0])[:-1]]).astype(np.uint32)
                c.check(run.L.shp_renumber_dev(c.handle, run.bufs.d_out, case.nr * case.nc, stride,
                                               base.ctypes.data_as(ctypes.c_void_p), nt))
                assert int(counts[:, 0].sum()) == m.maxSegId
                _check_outputs(run, m, m.maxSegId)
            run.ok = True
        finally:
            run.close()
