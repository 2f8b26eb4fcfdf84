"""The world-1 overhead of the distributed spatial statistics: distributed.deviceSpatialStats (one rank, the
whole raster as its rows: local pass, classification, record packing, no exchange) against the one-GPU
spatial statistics of the same device-resident raster (shp_spatialstats_dev) and against
tilingstats.calcPerSegmentSpatialStats on host arrays (which adds the uploads), for each built-in function, on
a C5-like label raster of 4 x 8-pixel blocks and one uint16 band.  Checks that the three agree bit for bit.

    python tools/perf_spatial_dist.py [N=8000] [REPS=5]

Nothing here measures multi-GPU scaling: one process, one GPU."""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pyshepseg_amd import comm as C, distributed, tiling, tilingstats as ts, _lib  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
(BH, BW, NULL) = (4, 8, 0)
c = _lib.ctx()
L = c._L
ras = tiling.DeviceRaster.synth(11, 1, N, N)
d_seg = ctypes.c_void_p()
c.check(L.shp_dev_alloc(c.handle, N * N * 4, ctypes.byref(d_seg)))
S = ctypes.c_uint32(0)
c.check(L.shp_dev_block_labels(c.handle, N, N, BH, BW, d_seg, ctypes.byref(S)))
S = S.value
seg = np.empty((N, N), dtype=np.uint32)
band = np.empty((N, N), dtype=np.uint16)
c.check(L.shp_dev_download(c.handle, _lib.ptr(seg), d_seg, seg.nbytes))
c.check(L.shp_dev_download(c.handle, _lib.ptr(band), ctypes.c_void_p(ras.ptr), band.nbytes))
hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.uint32)
hist[0] = 0
print('%d x %d labels, %d segments, band uint16 (nodata %d: %.3f %% of pixels)'
      % (N, N, S, NULL, 100.0 * (band == NULL).mean()))
R, I = ts.GFT_Real, ts.GFT_Integer
CASES = [('meancoord', ts.userFuncMeanCoord, [300000.0, 10.0, 0.0, 7000000.0, 0.0, -10.0], [R, R]),
         ('edges 4-conn', ts.userFuncNumEdgePixels, True, [I]),
         ('edges 8-conn', ts.userFuncNumEdgePixels, False, [I]),
         ('variogram 5', ts.userFuncVariogram, 5, [R] * 5)]
comm = C.LocalComm()


def best(f):
    f()                                         # warm-up: code objects, workspace growth
    ts_ = []
    for _ in range(REPS):
        c.check(L.shp_sync(c.handle))
        t = time.perf_counter()
        r = f()
        c.check(L.shp_sync(c.handle))
        ts_.append(time.perf_counter() - t)
    return r, min(ts_), float(np.median(ts_))


for (name, fn, prm, types) in CASES:
    nInt = sum(1 for t in types if t == I)
    nFloat = len(types) - nInt
    params = np.zeros(6, dtype=np.float64)
    pv = np.atleast_1d(np.asarray(prm, dtype=np.float64))
    params[:len(pv)] = pv

    def one():
        ic = np.zeros((max(nInt, 1), S + 1), dtype=np.int64)
        fc = np.zeros((max(nFloat, 1), S + 1), dtype=np.float32)
        c.check(L.shp_spatialstats_dev(c.handle, d_seg, ctypes.c_void_p(ras.ptr), 2, N, N, S, NULL, fn.funcId,
                                       _lib.ptr(params), -9999, nInt, nFloat, _lib.ptr(ic), _lib.ptr(fc)))
        return ic[:nInt], fc[:nFloat]

    def dist():
        r = distributed.deviceSpatialStats(c, comm, d_seg.value, ras.ptr, 2, N, N, (0, N), hist, types, fn, prm,
                                           -9999, NULL)
        return r[0], r[1]

    def host():
        return ts.calcPerSegmentSpatialStats(seg, band, types, fn, prm, NULL, maxSegId=S)
    (a, ta, ma) = best(one)
    (b, tb, mb) = best(dist)
    (h, th, mh) = best(host)
    for (x, y) in ((a, b), (a, h)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)), name
    print('%-13s one GPU (device rasters) %8.2f ms | distributed world 1 %8.2f ms (x%.2f) | '
          'calcPerSegmentSpatialStats (host arrays) %8.2f ms   [best of %d; medians %.2f / %.2f / %.2f]'
          % (name, ta * 1e3, tb * 1e3, tb / ta, th * 1e3, REPS, ma * 1e3, mb * 1e3, mh * 1e3))
c.check(L.shp_dev_free(c.handle, d_seg))
ras.free()
