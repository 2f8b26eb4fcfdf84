"""Per-segment depths on the label raster of one synthetic tile, of a tiled mosaic and of one label of the mosaic's size.

    python tools/perf_depths.py [--tile-size 4096] [--mosaic-size 16384] [--repeats 3] [--skip-tile] [--skip-mosaic] [--skip-one] [--out results.jsonl]

Three label rasters, all in HBM and read in place (the first two are tools/perf_shapes.py's and tools/perf_outlines.py's):
  tile       the labels of --tile-size x --tile-size synthetic 3-band imagery segmented as ONE tile
  mosaic     the labels of --mosaic-size x --mosaic-size imagery segmented in tiles of 4096 with 1024 overlap
  one_label  --mosaic-size x --mosaic-size pixels of label 1: every row run is as long as the raster is wide
Printed, each the median of --repeats calls after one untimed call (a JSON line per raster):
  wall_ms        depths.calcSegmentDepths(labels, maxSegId=..., coreAreas=two) from the call to the columns on the host
  device_ms      the library's events round its kernels, and steps_device_ms its split: columns (the column step),
                 window (the row step's window), envelope (the marked runs and their lower envelopes), reduce (the table)
  deferred_pixels    the pixels the window left to the envelope
  shapes_device_ms, trace_device_ms   shapes.calcSegmentShapes(...).deviceMs and the plain
                 outlines.traceSegmentOutlines(...).deviceMs on the same labels, as yardsticks
The untimed call is checked against the shape table: the depth-0 core is ``area``, the depth-1 core ``area - edgePixels``,
and every id with pixels has an interior pixel; the one-label raster's deepest pixel is half its side deep.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np


class Resident(object):
    """labels put into device memory, handed over as a segmentation kept on the device hands over its own"""
    def __init__(self, seg, maxSegId):
        from pyshepseg_amd import _lib
        self.c = _lib.ctx()
        self.p = ctypes.c_void_p()
        self.c.check(self.c._L.shp_dev_alloc(self.c.handle, seg.nbytes, ctypes.byref(self.p)))
        self.c.check(self.c._L.shp_dev_upload(self.c.handle, self.p, seg.ctypes.data_as(ctypes.c_void_p), seg.nbytes))
        self.outDev = (self.p.value, seg.shape[0], seg.shape[1], seg.nbytes)
        self.maxSegId = maxSegId

    def free(self):
        self.c.check(self.c._L.shp_dev_free(self.c.handle, self.p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tile-size', type=int, default=4096)
    ap.add_argument('--mosaic-size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--skip-tile', action='store_true')
    ap.add_argument('--skip-mosaic', action='store_true')
    ap.add_argument('--skip-one', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyshepseg_amd import depths, outlines, shapes, tiling
    out = open(a.out, 'a') if a.out else None
    cores = [('core0', 0), ('core1', 1)]

    def measure(what, labels, nrows, ncols, maxSegId):
        (wall, dev, steps) = ([], [], [])
        for rep in range(-1, a.repeats):
            t = time.perf_counter()
            r = depths.calcSegmentDepths(labels, maxSegId=maxSegId, coreAreas=cores)
            if rep >= 0:
                wall.append((time.perf_counter() - t) * 1e3)
                dev.append(r.deviceMs)
                steps.append(r.deviceStepsMs)
            else:
                s = shapes.calcSegmentShapes(labels, maxSegId=maxSegId)
                assert np.array_equal(r.columns['core0'], s.columns['area'])
                assert np.array_equal(r.columns['core1'], s.columns['area'] - s.columns['edgePixels'])
                assert np.array_equal(r.columns['maxDepth2'] > 0, s.columns['area'] > 0)
                if what == 'one_label':
                    assert r.columns['maxDepth2'].tolist() == [0, (min(nrows, ncols) // 2) ** 2]
        n = max(2, a.repeats)
        sh = [shapes.calcSegmentShapes(labels, maxSegId=maxSegId).deviceMs for _rep in range(n)][1:]
        tr = [outlines.traceSegmentOutlines(labels, maxSegId=maxSegId).deviceMs for _rep in range(n)][1:]
        line = json.dumps(dict(
            what=what, rows=nrows, cols=ncols, runs=len(wall), segments=maxSegId,
            wall_ms=round(statistics.median(wall), 1), wall_min_ms=round(min(wall), 1), wall_max_ms=round(max(wall), 1),
            device_ms=round(statistics.median(dev), 2), device_min_ms=round(min(dev), 2), device_max_ms=round(max(dev), 2),
            steps_device_ms={k: round(statistics.median(st[k] for st in steps), 3) for k in steps[0]},
            deferred_pixels=r.deferredPixels, deepest2=int(r.columns['maxDepth2'].max()),
            shapes_device_ms=round(statistics.median(sh), 2), trace_device_ms=round(statistics.median(tr), 2),
            steps_s={k: round(v, 4) for (k, v) in r.timings.items()}))
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    for (what, m, skip) in (('tile', a.tile_size, a.skip_tile), ('mosaic', a.mosaic_size, a.skip_mosaic)):
        if skip:
            continue
        ras = tiling.DeviceRaster.synth(3, 3, m, m)
        try:
            cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=4)
            t = time.perf_counter()
            rd = tiling.doTiledShepherdSegmentation(ras, tiling._KEEP_ON_DEVICE, tileSize=4096, overlapSize=1024,
                                                    minSegmentSize=50, numClusters=60, fixedKMeansInit=True,
                                                    concurrencyCfg=cfg)
            try:
                print('%s: %d segments, segmented in %.1f s' % (what, rd.maxSegId, time.perf_counter() - t), flush=True)
                measure(what, rd, m, m, rd.maxSegId)
            finally:
                tiling.freeDeviceOutput(rd)
        finally:
            ras.free()
    if not a.skip_one:
        m = a.mosaic_size
        one = Resident(np.ones((m, m), dtype=np.uint32), 1)
        try:
            measure('one_label', one, m, m, 1)
        finally:
            one.free()


if __name__ == '__main__':
    main()
