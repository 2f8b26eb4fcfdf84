"""Timings of user-defined spatial statistics on row shards (distributed.deviceSpatialStats with a user function;
pyshepseg_amd/csrc/dsegpoints.h), on a device-resident N x N raster of 8 x 8 block labels (shp_dev_block_labels)
and one synthetic uint16 band:

  device steps   for W = 1, 2, 4 row shards played one after the other on ONE GPU (each rank a context of its own;
                 shard boundaries 3 rows past a multiple of 8, so every boundary cuts a row of blocks):
                 shp_dsegpoints_build_dev per rank (local build, classification, record pack; synchronised), the
                 exchange played as device copies into one gathered buffer, shp_dsegpoints_merge_dev per rank --
                 against the one-GPU shp_segpoints_build_dev of the whole raster -- and the records per boundary;
  whole call     wall time of deviceSpatialStats with a trivial Python user function: world 1 in this process, then
                 2 and 4 socket ranks (processes) sharing GPU 0; a rank's time is from its first collective to its
                 return, the figure the slowest rank's.

    python tools/perf_spatial_userfunc_dist.py [N=16000] [REPS=3]"""
import ctypes
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pyshepseg_amd import comm as C, distributed, tiling, tilingstats as ts, _lib  # noqa: E402

NULL = 0
TILE = 1024


def raster(c, N):
    L = c._L
    ras = tiling.DeviceRaster.synth(11, 1, N, N)
    d_seg = ctypes.c_void_p()
    c.check(L.shp_dev_alloc(c.handle, N * N * 4, ctypes.byref(d_seg)))
    S = ctypes.c_uint32(0)
    c.check(L.shp_dev_block_labels(c.handle, N, N, 8, 8, d_seg, ctypes.byref(S)))
    S = S.value
    hist = np.zeros(S + 1, np.uint32)
    c.check(L.shp_histogram_dev(c.handle, d_seg, N * N, N, S, _lib.ptr(hist)))
    hist[0] = 0
    return ras, d_seg, S, hist


def shards(N, W):
    cuts = [0] + [r * N // W + 3 for r in range(1, W)] + [N]
    return [(cuts[r], cuts[r + 1]) for r in range(W)]


def trivial(pts, imgNullVal, intArr, floatArr, userParam):
    intArr[0] = len(pts)


def deviceSteps(N, REPS):
    c = _lib.Context()
    L = c._L
    (ras, d_seg, S, hist) = raster(c, N)
    dt = _lib.SHP_DTYPES[np.dtype(np.uint16)]
    d_hist = ctypes.c_void_p()
    c.check(L.shp_dev_alloc(c.handle, hist.nbytes, ctypes.byref(d_hist)))
    c.check(L.shp_dev_upload(c.handle, d_hist, _lib.ptr(hist), hist.nbytes))
    npts = ctypes.c_int64(0)
    best = 1e30
    for _r in range(REPS):
        t0 = time.perf_counter()
        c.check(L.shp_segpoints_build_dev(c.handle, d_seg, ctypes.c_void_p(ras.ptr), dt, N, N, S, NULL, TILE,
                                          ctypes.byref(npts)))
        best = min(best, time.perf_counter() - t0)
    print('%d x %d labels (8 x 8 blocks), %d segments, %d points; one-GPU shp_segpoints_build_dev: %.2f ms'
          % (N, N, S, npts.value, 1e3 * best, ))
    for W in (1, 2, 4):
        rr = shards(N, W)
        pcs = [_lib.Context() for _r in range(W)]
        tb = [1e30] * W
        tm = [1e30] * W
        tx = 1e30
        for _rep in range(REPS):
            recs = []
            for (r, (lo, hi)) in enumerate(rr):
                lh = np.zeros(S + 1, np.uint32)
                lp = np.zeros(S + 1, np.uint32)
                (pRec, nRec) = (ctypes.c_void_p(), ctypes.c_int64(0))
                t0 = time.perf_counter()
                pcs[r].check(L.shp_dsegpoints_build_dev(
                    pcs[r].handle, ctypes.c_void_p(d_seg.value + lo * N * 4), ctypes.c_void_p(ras.ptr + lo * N * 2),
                    dt, hi - lo, N, lo, N, S, NULL, TILE, d_hist, _lib.ptr(lh), _lib.ptr(lp), ctypes.byref(pRec),
                    ctypes.byref(nRec)))
                tb[r] = min(tb[r], time.perf_counter() - t0)
                recs.append((pRec.value, nRec.value))
            slot = max(n for (_p, n) in recs)
            nb = max(slot * 24, 24)
            d_all = ctypes.c_void_p()
            c.check(L.shp_dev_alloc(c.handle, W * nb, ctypes.byref(d_all)))
            t0 = time.perf_counter()
            for (r, (p, n)) in enumerate(recs):
                if n:
                    c.check(L.shp_dev_copy(c.handle, ctypes.c_void_p(d_all.value + r * nb), ctypes.c_void_p(p),
                                           n * 24))
            tx = min(tx, time.perf_counter() - t0)
            cnts = np.array([n for (_p, n) in recs], np.uint32)
            for r in range(W):
                (a, b) = distributed.idRange(r, W, S)
                merged = np.zeros(max(b - a, 1), np.uint32)
                nm = ctypes.c_int64(0)
                t0 = time.perf_counter()
                pcs[r].check(L.shp_dsegpoints_merge_dev(pcs[r].handle, d_all, slot, W, _lib.ptr(cnts), a, b,
                                                        _lib.ptr(merged), ctypes.byref(nm)))
                tm[r] = min(tm[r], time.perf_counter() - t0)
            c.check(L.shp_dev_free(c.handle, d_all))
        print('W=%d shards %s: build+pack per rank %s ms (max %.2f); exchange as device copies %.3f ms; '
              'merge per rank %s ms; records %d (%.0f per boundary, %.2f MB per boundary)'
              % (W, rr, ' '.join('%.2f' % (1e3 * t) for t in tb), 1e3 * max(tb), 1e3 * tx,
                 ' '.join('%.2f' % (1e3 * t) for t in tm), int(cnts.sum()), cnts.sum() / max(W - 1, 1),
                 24.0 * cnts.sum() / max(W - 1, 1) / 1e6))
        for pc in pcs:
            pc.close()
    c.check(L.shp_dev_free(c.handle, d_hist))
    c.check(L.shp_dev_free(c.handle, d_seg))
    ras.free()
    c.close()


def oneRank(comm, N):
    """deviceSpatialStats of this rank's rows with the trivial function: (seconds, calls)"""
    c = _lib.Context()
    (ras, d_seg, S, hist) = raster(c, N)
    (lo, hi) = shards(N, comm.world)[comm.rank]
    dcomm = comm if getattr(comm, 'onDevice', False) else C.HostStagedDev(comm, c)
    fn = ts.spatialUserFunc(trivial)
    info = {}
    comm.barrier()
    t0 = time.perf_counter()
    (ic, _fc, _n, _h) = distributed.deviceSpatialStats(
        c, dcomm, d_seg.value + lo * N * 4, ras.ptr + lo * N * 2, 2, N, N, (lo, hi), hist, [ts.GFT_Integer], fn, None,
        -9999, NULL, info=info)
    dt = time.perf_counter() - t0
    c.check(c._L.shp_dev_free(c.handle, d_seg))
    ras.free()
    c.close()
    return dt, info


def wholeCall(N):
    (t1, info) = oneRank(C.LocalComm(), N)
    print('whole call, world 1 (this process): %.2f s, %d calls' % (t1, info['calls']))
    for W in (2, 4):
        tmp = tempfile.mkdtemp()
        procs = []
        for r in range(W):
            env = dict(os.environ, SHEPSEG_LAUNCH_NONCE='perf%d' % W, RANK=str(r), LOCAL_RANK=str(r),
                       WORLD_SIZE=str(W), MASTER_ADDR='127.0.0.1', MASTER_PORT='0', SHEPSEG_DEVICE='0',
                       SHEPSEG_COMM_DIR=os.path.join(tmp, 'comm'))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), '--rank', str(N)], env=env,
                                          stdout=subprocess.PIPE, text=True))
        outs = [p.communicate(timeout=900)[0] for p in procs]
        if any(p.returncode for p in procs):
            raise SystemExit('a rank failed: %s' % [p.returncode for p in procs])
        res = [tuple(float(x) for x in o.split()[-3:]) for o in outs]
        print('whole call, %d socket ranks sharing GPU 0: %.2f s (ranks %s s; calls %s; straddlers %d)'
              % (W, max(r[0] for r in res), ' '.join('%.2f' % r[0] for r in res),
                 ' '.join('%d' % r[1] for r in res), int(res[0][2])))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--rank':
        comm = C.SocketComm()
        (t, info) = oneRank(comm, int(sys.argv[2]))
        comm.close()
        print('%f %d %d' % (t, info['calls'], info['straddlers']))
        sys.exit(0)
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 16000
    REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    deviceSteps(N, REPS)
    wholeCall(N)
