"""Segment neighbours and border lengths at the C5 size and on a real segmentation.

    python tools/perf_neighbours.py [--size 40000] [--seg-size 8192] [--repeats 3] [--skip-blocks] [--skip-seg] [--out results.jsonl]

Two label rasters, both resident in HBM and read in place, each with 4- and 8-connectivity:
  blocks   --size x --size labels of 4 x 8-pixel blocks (shp_dev_block_labels, the C5 workload's block shape:
           50 M segments at 40000), every table checked against the closed form of a block grid
  segment  the labels a tiled segmentation of --seg-size x --seg-size synthetic 3-band imagery keeps on the device
Printed, each the median of --repeats calls after one untimed call (a JSON line per figure):
  wall_ms        neighbours.findSegmentNeighbours from the call to the three host arrays (the download included)
  device_ms      the library's events around the patch kernels and the finish (sort, reduce, CSR)
  pairs_seen / records_sorted   differing pixel pairs met / records the patches handed to the global sort
  hbm_read_floor the labels' bytes over device_ms as a fraction of ONE read of the raster at 8 TB/s: nothing did this
                 work before, so the read of the input is the floor it is held against
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


def check_block_grid(t, n, four):
    """the table of an n x n raster of BH x BW blocks numbered row-major from 1"""
    (nbr, nbc) = (n // BH, n // BW)
    assert t.maxSegId == nbr * nbc
    deg = np.diff(t.offsets)[1:].reshape(nbr, nbc)
    rows = np.full(nbr, 2)
    rows[[0, -1]] = 1
    cols = np.full(nbc, 2)
    cols[[0, -1]] = 1
    want = rows[:, None] + cols[None, :]
    if not four:
        want = want + rows[:, None] * cols[None, :]
    assert np.array_equal(deg, want), 'degrees differ from the block grid\'s'
    # every block but the last of a row touches the next along BH pixel pairs (8-connected: + 2 (BH - 1) diagonals)
    (ids, lens) = t.neighboursOf(1)
    e = BH if four else BH + 2 * (BH - 1)
    s = BW if four else BW + 2 * (BW - 1)
    if four:
        assert ids.tolist() == [2, nbc + 1] and lens.tolist() == [e, s]
    else:
        assert ids.tolist() == [2, nbc + 1, nbc + 2] and lens.tolist() == [e, s, 1]
    total = (nbr * (nbc - 1) * e + (nbr - 1) * nbc * s + (0 if four else 2 * (nbr - 1) * (nbc - 1)))
    assert int(t.borderLengths.sum()) == 2 * total and t.pairsSeen == total


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
    from pyshepseg_amd import neighbours, tiling, _lib
    c = _lib.ctx()
    L = c._L
    out = open(a.out, 'a') if a.out else None

    def measure(what, labels, nrows, ncols, check=None):
        for four in (True, False):
            (wall, dev) = ([], [])
            for rep in range(-1, a.repeats):
                t = time.perf_counter()
                r = neighbours.findSegmentNeighbours(labels, fourConnected=four)
                if rep >= 0:
                    wall.append((time.perf_counter() - t) * 1e3)
                    dev.append(r.deviceMs)
                elif check is not None:
                    check(r, four)
            ms = statistics.median(dev)
            line = json.dumps(dict(
                what=what, rows=nrows, cols=ncols, fourConnected=four, runs=len(wall), segments=r.maxSegId,
                entries=len(r.neighbours), wall_ms=round(statistics.median(wall), 1), wall_min_ms=round(min(wall), 1),
                wall_max_ms=round(max(wall), 1), device_ms=round(ms, 2), device_min_ms=round(min(dev), 2),
                device_max_ms=round(max(dev), 2), pairs_seen=r.pairsSeen, records_sorted=r.recordsSorted,
                hbm_read_floor=round((4.0 * nrows * ncols / HBM_PEAK) / (ms / 1e3), 4),
                steps_s={k: round(v, 4) for (k, v) in r.timings.items()}))
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
            measure('blocks', ResidentLabels(d_seg.value, n, n), n, n, lambda r, four: check_block_grid(r, n, four))
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
                measure('segment', rd, m, m)
            finally:
                tiling.freeDeviceOutput(rd)
        finally:
            ras.free()


if __name__ == '__main__':
    main()
