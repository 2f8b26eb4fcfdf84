"""Helpers of tests/test_gpu_spatial_distributed.py: row shards of one raster played by threads of one process
on one GPU, with an in-process stand-in for RcclComm's device collectives."""
import ctypes
import threading

import numpy as np


class ThreadDevComm(object):
    """`world` threads of one process, one GPU: allgather_obj through shared slots, allgather_dev as device to
    device copies, allreduce_dev_i64 adds through the host (test data is small)."""
    onDevice = True

    def __init__(self, rank, world, shared):
        (self.rank, self.world, self.sh) = (rank, world, shared)
        if 'bar' not in shared:                # (made once, before the rank threads start)
            shared['bar'] = threading.Barrier(world, timeout=60)
            shared['slots'] = [None] * world
        self.c = None

    def _xchg(self, v):
        self.sh['bar'].wait()
        self.sh['slots'][self.rank] = v
        self.sh['bar'].wait()
        out = list(self.sh['slots'])
        self.sh['bar'].wait()
        return out

    def allgather_obj(self, obj):
        return self._xchg(obj)

    def allgather_dev(self, d_send, d_recv, nbytes):
        ptrs = self._xchg(d_send)
        for (r, p) in enumerate(ptrs):
            self.c.check(self.c._L.shp_dev_copy(self.c.handle, ctypes.c_void_p(d_recv + r * nbytes),
                                                ctypes.c_void_p(p), nbytes))
        self.sh['bar'].wait()                  # nobody frees a send buffer another rank still reads

    def allreduce_dev_i64(self, d_buf, count):
        from pyshepseg_amd import _lib
        mine = np.empty(count, dtype=np.int64)
        self.c.check(self.c._L.shp_dev_download(self.c.handle, _lib.ptr(mine), ctypes.c_void_p(d_buf), mine.nbytes))
        tot = np.sum(self._xchg(mine), axis=0, dtype=np.int64)
        self.c.check(self.c._L.shp_dev_upload(self.c.handle, ctypes.c_void_p(d_buf), _lib.ptr(tot), tot.nbytes))


def runShards(seg, band, ranges, work, timeout=300):
    """One thread per rank: rank r holds rows ranges[r] of seg / band in device memory of a context of its own
    and returns work(ctx, comm, d_seg, d_band, rowRange).  Returns (results, errors) per rank; a rank stranded
    in a collective by another one's exception gets BrokenBarrierError when the barrier times out (60 s)."""
    from pyshepseg_amd import _lib
    world = len(ranges)
    shared = {}
    (results, errors) = ([None] * world, [None] * world)
    ThreadDevComm(0, world, shared)          # the barrier exists before any thread runs

    def rank(r):
        c = None
        bufs = []
        try:
            c = _lib.Context()
            comm = ThreadDevComm(r, world, shared)
            comm.c = c
            (lo, hi) = ranges[r]
            ptrs = []
            for a in (seg, band):
                part = np.ascontiguousarray(a[lo:hi])
                p = ctypes.c_void_p()
                c.check(c._L.shp_dev_alloc(c.handle, max(part.nbytes, 16), ctypes.byref(p)))
                bufs.append(p)
                if part.nbytes:
                    c.check(c._L.shp_dev_upload(c.handle, p, _lib.ptr(part), part.nbytes))
                ptrs.append(p.value)
            results[r] = work(c, comm, ptrs[0], ptrs[1], (lo, hi))
        except BaseException as e:      # noqa: B902
            errors[r] = e               # (a rank left waiting for this one breaks the barrier at its timeout)
        finally:
            if c is not None:
                for p in bufs:
                    c._L.shp_dev_free(c.handle, p)
                c.close()
    th = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout)
    assert not any(t.is_alive() for t in th), 'a rank is still running after %d s' % timeout
    return results, errors


def blockRaster(rng, nr, nc, dtype, nullv):
    """Labels: blocks of a coarse random field plus vertical streaks (segments that cross every shard boundary),
    2 % unlabelled pixels; band: random values with 10 % nodata and one segment (id 5) that is all nodata.
    Returns (seg, band, S) with S three above the largest id (ids nobody holds)."""
    base = rng.integers(1, 40, size=(nr // 7 + 2, nc // 5 + 1))
    seg = np.kron(base, np.ones((7, 5), dtype=np.int64))[:nr, :nc]
    seg = seg + (np.arange(nc)[None, :] // 13) * 40
    streak = (np.arange(nc) % 17) == 3
    seg[:, streak] = 1000 + np.arange(nc)[streak][None, :] // 17
    seg = seg.astype(np.uint32)
    seg[rng.random((nr, nc)) < 0.02] = 0
    info = np.iinfo(dtype)
    band = rng.integers(max(info.min, -3000), min(info.max, 3000) + 1, size=(nr, nc)).astype(dtype)
    band[rng.random((nr, nc)) < 0.1] = nullv
    band[seg == 5] = nullv
    return seg, band, int(seg.max()) + 3
