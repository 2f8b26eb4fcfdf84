"""Timings of the per-segment point lists behind user-defined spatial statistics (pyshepseg_amd/csrc/segpoints.h):

  device build   shp_segpoints_build_dev on a device-resident N x N raster (block labels of 8 x 8 pixels from
                 shp_dev_block_labels, one synthetic uint16 band): points/s, and GB/s of the two raster passes
                 (4-byte label + 2-byte value per pixel, read twice) against HBM;
  emission       shp_segpoints_emit of every batch into pinned host memory: 16-byte records/s (PCIe-bound);
  batch consumer tilingstats.iterSegmentPoints on the same raster downloaded, with a vectorised per-batch reduction;
  per-segment    calcPerSegmentSpatialStats with a trivial Python callback on an E x E crop (one call per segment).

    python tools/perf_spatial_points.py [N=16000] [E=4000] [REPS=3]"""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pyshepseg_amd import tiling, tilingstats as ts, _lib  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 16000
E = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
NULL = 0
c = _lib.Context()
L = c._L
ras = tiling.DeviceRaster.synth(11, 1, N, N)
d_seg = ctypes.c_void_p()
c.check(L.shp_dev_alloc(c.handle, N * N * 4, ctypes.byref(d_seg)))
S = ctypes.c_uint32(0)
c.check(L.shp_dev_block_labels(c.handle, N, N, 8, 8, d_seg, ctypes.byref(S)))
S = S.value
d_band = ctypes.c_void_p(ras.ptr)
dt = _lib.SHP_DTYPES[np.dtype(np.uint16)]
counts = np.zeros(S + 1, np.uint32)
t0 = time.perf_counter()
c.check(L.shp_segpoints_count_dev(c.handle, d_seg, d_band, dt, N, N, S, NULL, _lib.ptr(counts)))
t_count = time.perf_counter() - t0
total = int(counts.sum(dtype=np.int64))
print('%d x %d labels, %d segments, %d points (%.2f %% nodata); count %.1f ms'
      % (N, N, S, total, 100.0 * (1 - total / float(N * N)), 1e3 * t_count))
batches = ts.planPointBatches(counts, ts.POINTS_BATCH)
cap = ts.POINTS_BATCH + int(counts.max())
hbuf = ctypes.c_void_p()             # (before the build: emission must follow it directly)
c.check(L.shp_host_alloc(c.handle, cap * 16, ctypes.byref(hbuf)))
npts = ctypes.c_int64(0)
best = 1e30
for _r in range(REPS):
    t0 = time.perf_counter()
    c.check(L.shp_segpoints_build_dev(c.handle, d_seg, d_band, dt, N, N, S, NULL, 1024, ctypes.byref(npts)))
    best = min(best, time.perf_counter() - t0)
assert npts.value == total
print('device build (tile 1024): %.1f ms  %.2f Gpoints/s  %.0f GB/s of raster passes'
      % (1e3 * best, total / best / 1e9, 2 * N * N * 6 / best / 1e9))
n = ctypes.c_int64(0)
t0 = time.perf_counter()
for (lo, hi) in batches:
    offs = np.empty(hi - lo + 1, np.int64)
    c.check(L.shp_segpoints_emit(c.handle, lo, hi, _lib.ptr(offs), hbuf, cap, ctypes.byref(n)))
t_emit = time.perf_counter() - t0
print('emission: %d batches  %.1f ms  %.2f Gpoints/s  %.1f GB/s of records to the host'
      % (len(batches), 1e3 * t_emit, total / t_emit / 1e9, 16.0 * total / t_emit / 1e9))
c.check(L.shp_host_free(c.handle, hbuf))
seg = np.empty((N, N), np.uint32)
band = np.empty((N, N), np.uint16)
c.check(L.shp_dev_download(c.handle, _lib.ptr(seg), d_seg, seg.nbytes))
c.check(L.shp_dev_download(c.handle, _lib.ptr(band), d_band, band.nbytes))
c.check(L.shp_dev_free(c.handle, d_seg))
ras.free()
c.close()

t0 = time.perf_counter()
acc = 0
for (ids, offs, pts) in ts.iterSegmentPoints(seg, band, NULL, maxSegId=S):
    if len(pts):
        acc += int(np.add.reduceat(pts.val, offs[:-1][offs[:-1] < len(pts)]).sum())
t_iter = time.perf_counter() - t0
print('batch consumer (iterSegmentPoints + per-batch reduceat): %.2f s  %.1f Mpoints/s end to end'
      % (t_iter, total / t_iter / 1e6))
crop_s, crop_b = seg[:E, :E], band[:E, :E]
nseg = len(np.unique(crop_s[crop_b != NULL]))
t0 = time.perf_counter()
ic, _fc = ts.calcPerSegmentSpatialStats(crop_s, crop_b, [ts.GFT_Integer], ts.spatialUserFunc(lambda pts, *a: None), None, NULL)
t_cb = time.perf_counter() - t0
print('per-segment callback (%d x %d, %d segments): %.2f s  %.1f us per segment'
      % (E, E, nseg, t_cb, 1e6 * t_cb / max(nseg, 1)))
