"""Per-segment shape attributes at the C5 size and on a real segmentation.

    python tools/perf_shapes.py [--size 40000] [--seg-size 8192] [--repeats 3] [--skip-blocks] [--skip-seg] [--out results.jsonl]

Two label rasters, both resident in HBM and read in place (tools/perf_neighbours.py's):
  blocks   --size x --size labels of 4 x 8-pixel blocks (shp_dev_block_labels: 50 M segments at 40000), every column
           checked against the closed form of a block grid
  segment  the labels a tiled segmentation of --seg-size x --seg-size synthetic 3-band imagery keeps on the device
Printed, each the median of --repeats calls after one untimed call (a JSON line per raster):
  wall_ms        shapes.calcSegmentShapes(labels, maxSegId=...) from the call to the columns on the host (the download
                 of 88 bytes per id and the derived columns in numpy included)
  device_ms      the library's events around the table's initialisation, the patch kernels and the finish
  hbm_read_floor the labels' bytes over device_ms as a fraction of ONE read of the raster at 8 TB/s
  label_max_device_ms   the reduction that finds the largest label when no maxSegId is given (one more read)
  neighbours4_device_ms findSegmentNeighbours(fourConnected=True).deviceMs on the same labels, for comparison
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

BH, BW = 4, 8
HBM_PEAK = 8.0e12


class ResidentLabels(object):
    def __init__(self, ptr, nrows, ncols):
        self.outDev = (ptr, nrows, ncols, nrows * ncols * 4)


def check_block_grid(s, n):
    """the columns of an n x n raster of BH x BW blocks numbered row-major from 1"""
    (nbr, nbc) = (n // BH, n // BW)
    assert s.maxSegId == nbr * nbc
    cols = s.columns
    assert np.all(cols['area'][1:] == BH * BW) and np.all(cols['perimeter'][1:] == 2 * (BH + BW))
    assert np.all(cols['edgePixels'][1:] == BH * BW - (BH - 2) * (BW - 2))
    assert int(cols['outerBorder'].sum()) == 4 * n
    (by, bx) = np.divmod(np.arange(nbr * nbc, dtype=np.int64), nbc)
    assert np.array_equal(cols['rowMin'][1:], by * BH) and np.array_equal(cols['colMax'][1:], bx * BW + BW - 1)
    assert np.array_equal(cols['centroidRow'][1:], by * BH + (BH - 1) / 2.0)
    assert np.array_equal(cols['centroidCol'][1:], bx * BW + (BW - 1) / 2.0)
    assert np.allclose(cols['elongation'][1:], BW / BH, rtol=1e-12, atol=0) and np.all(cols['bboxFill'][1:] == 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=40000)
    ap.add_argument('--seg-size', type=int, default=8192)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--skip-blocks', action='store_true')
    ap.add_argument('--skip-seg', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyshepseg_amd import neighbours, shapes, tiling, _lib
    c = _lib.ctx()
    L = c._L
    out = open(a.out, 'a') if a.out else None

    def measure(what, labels, nrows, ncols, maxSegId, check=None):
        (wall, dev) = ([], [])
        for rep in range(-1, a.repeats):
            t = time.perf_counter()
            r = shapes.calcSegmentShapes(labels, maxSegId=maxSegId)
            if rep >= 0:
                wall.append((time.perf_counter() - t) * 1e3)
                dev.append(r.deviceMs)
            elif check is not None:
                check(r)
        steps = {k: round(v, 4) for (k, v) in r.timings.items()}
        del r
        top = ctypes.c_uint32(0)
        lm = ctypes.c_double(0)
        c.check(L.shp_shape_label_max_dev(c.handle, ctypes.c_void_p(labels.outDev[0]), nrows * ncols, ctypes.byref(top),
                                          ctypes.byref(lm)))
        assert top.value == maxSegId
        nb = [neighbours.findSegmentNeighbours(labels, fourConnected=True, maxSegId=maxSegId).deviceMs
              for _rep in range(max(2, a.repeats))][1:]
        ms = statistics.median(dev)
        line = json.dumps(dict(
            what=what, rows=nrows, cols=ncols, runs=len(wall), segments=maxSegId,
            wall_ms=round(statistics.median(wall), 1), wall_min_ms=round(min(wall), 1), wall_max_ms=round(max(wall), 1),
            device_ms=round(ms, 2), device_min_ms=round(min(dev), 2), device_max_ms=round(max(dev), 2),
            hbm_read_floor=round((4.0 * nrows * ncols / HBM_PEAK) / (ms / 1e3), 4),
            label_max_device_ms=round(lm.value, 2), neighbours4_device_ms=round(statistics.median(nb), 2),
            steps_s=steps))
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    if not a.skip_blocks:
        n = a.size
        if n % BH or n % BW:
            raise SystemExit('--size must be a multiple of %d' % BW)
        d_seg = ctypes.c_void_p()
        c.check(L.shp_dev_alloc(c.handle, n * n * 4, ctypes.byref(d_seg)))
        try:
            Sc = ctypes.c_uint32(0)
            c.check(L.shp_dev_block_labels(c.handle, n, n, BH, BW, d_seg, ctypes.byref(Sc)))
            measure('blocks', ResidentLabels(d_seg.value, n, n), n, n, (n // BH) * (n // BW),
                    lambda r: check_block_grid(r, n))
        finally:
            c.check(L.shp_dev_free(c.handle, d_seg))
    if not a.skip_seg:
        m = a.seg_size
        ras = tiling.DeviceRaster.synth(3, 3, m, m)
        try:
            cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=4)
            rd = tiling.doTiledShepherdSegmentation(ras, tiling._KEEP_ON_DEVICE, tileSize=4096, overlapSize=1024,
                                                    minSegmentSize=50, numClusters=60, fixedKMeansInit=True,
                                                    concurrencyCfg=cfg)
            try:
                print('segmentation: %d segments' % rd.maxSegId, flush=True)
                measure('segment', rd, m, m, rd.maxSegId)
            finally:
                tiling.freeDeviceOutput(rd)
        finally:
            ras.free()


if __name__ == '__main__':
    main()
