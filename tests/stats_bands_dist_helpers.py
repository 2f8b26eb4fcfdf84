"""Helpers of tests/test_gpu_stats_bands_dist.py (no tests here): a stand-in for RcclComm's device collectives
between the threads of one process, the two label fields of the several-band device-path test, and what numpy
counts in them."""
import ctypes
import threading

import numpy as np


class ThreadDevComm(object):
    """An in-process stand-in for RcclComm's device collectives: `world` threads of one process, one GPU.
    allgather_dev copies device to device, allreduce_dev_i64 adds through the host (test data is small)."""
    onDevice = True

    def __init__(self, rank, world, shared):
        (self.rank, self.world, self.sh) = (rank, world, shared)
        if 'bar' not in shared:                # (made once, before the rank threads start: a second barrier
            shared['bar'] = threading.Barrier(world)        # would strand whoever waits at the first)
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
            self.c.check(self.c._L.shp_dev_copy(self.c.handle, ctypes.c_void_p(d_recv + r * nbytes), ctypes.c_void_p(p), nbytes))
        self.sh['bar'].wait()                  # nobody frees a send buffer another rank still reads

    def allreduce_dev_i64(self, d_buf, count):
        from pyshepseg_amd import _lib
        mine = np.empty(count, dtype=np.int64)
        self.c.check(self.c._L.shp_dev_download(self.c.handle, _lib.ptr(mine), ctypes.c_void_p(d_buf), mine.nbytes))
        tot = np.sum(self._xchg(mine), axis=0, dtype=np.int64)
        self.c.check(self.c._L.shp_dev_upload(self.c.handle, ctypes.c_void_p(d_buf), _lib.ptr(tot), tot.nbytes))


def runRankThreads(world, body, timeout=300):
    """body(rank, comm, ctx) in `world` threads, each with a context and a ThreadDevComm of its own.  Returns
    (results, errors) by rank.  A thread that raises waits a moment for the others to leave their bodies too (an
    error every rank raises needs no help, and aborting the barrier while the others still wake from its last
    release would hand them BrokenBarrierError in place of their own error); if they do not, it aborts the barrier
    so that nobody waits for it.  Every thread is joined with a time limit (one still alive then is an error)."""
    import time
    from pyshepseg_amd import _lib
    shared, results, errors, left = {}, [None] * world, [None] * world, [False] * world

    def rank(r):
        c = None
        try:
            c = _lib.Context()
            comm = ThreadDevComm(r, world, shared)
            comm.c = c
            results[r] = body(r, comm, c)
            left[r] = True
        except BaseException as e:      # noqa: B902  (a dead rank must not leave the others at a barrier)
            errors[r] = e
            left[r] = True
            deadline = time.monotonic() + 5.0
            while not all(left) and time.monotonic() < deadline:
                time.sleep(0.01)
            if not all(left):
                try:
                    shared['bar'].abort()
                except Exception:
                    pass
        finally:
            if c is not None:
                c.close()
    ThreadDevComm(0, world, shared)          # the barrier exists before any thread runs
    th = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for (r, t) in enumerate(th):
        t.join(timeout)
        if t.is_alive():
            errors[r] = TimeoutError('rank thread %d did not return' % r)
    return results, errors


(NR, NC) = (203, 190)


def cutsOf(world):
    return [0] + [int(round(NR * (r + 1) / world)) for r in range(world)]


def labelField(kind, rng):
    """'A': 7 x 5 blocks of a coarse random field + 40 per 37 columns, 3 % zeros -- long vertical streaks, most ids
    straddle every cut.  'B': the same + 240 per 28 rows, so that most segments are whole on one rank.  Returns
    (seg uint32, S) with S = max + 3: some ids are held by nobody."""
    base = rng.integers(1, 40, size=(NR // 7 + 2, NC // 5 + 1))
    seg = np.kron(base, np.ones((7, 5), dtype=np.int64))[:NR, :NC]
    seg = seg + (np.arange(NC)[None, :] // 37) * 40
    if kind == 'B':
        seg = seg + 240 * (np.arange(NR)[:, None] // 28)
    seg = seg.astype(np.uint32)
    seg[rng.random((NR, NC)) < 0.03] = 0
    return seg, int(seg.max()) + 3


def countField(seg, S, world):
    """numpy's account of the field at this world size: dict of the straddling ids, their pixels, the straddlers
    per rank's id share, and the ids whole on each rank"""
    from pyshepseg_amd import distributed
    cuts = cutsOf(world)
    held = [set(np.unique(seg[cuts[r]:cuts[r + 1]]).tolist()) - {0} for r in range(world)]
    strad = set()
    for a in range(world):
        for b in range(a + 1, world):
            strad |= held[a] & held[b]
    shares = [distributed.idRange(r, world, S) for r in range(world)]
    return dict(strad=strad, pixels=int(np.isin(seg, sorted(strad)).sum()),
                perShare=[sum(1 for s in strad if lo <= s < hi) for (lo, hi) in shares],
                whole=[len(held[r] - strad) for r in range(world)], held=held)


def uploadRows(c, a):
    """rows of a host array in device memory of context c: a c_void_p the caller frees with shp_dev_free"""
    from pyshepseg_amd import _lib
    a = np.ascontiguousarray(a)
    d = ctypes.c_void_p()
    c.check(c._L.shp_dev_alloc(c.handle, max(a.nbytes, 16), ctypes.byref(d)))
    if a.nbytes:
        c.check(c._L.shp_dev_upload(c.handle, d, _lib.ptr(a), a.nbytes))
    return d
