"""Segment outlines on the label raster of one synthetic tile and of a tiled mosaic.

    python tools/perf_outlines.py [--tile-size 4096] [--mosaic-size 16384] [--repeats 3] [--eight] [--skip-tile] [--skip-mosaic] [--out results.jsonl]

Two label rasters, both kept in HBM by the segmentation and read in place (tools/perf_shapes.py's second raster):
  tile     the labels of --tile-size x --tile-size synthetic 3-band imagery segmented as ONE tile
  mosaic   the labels of --mosaic-size x --mosaic-size imagery segmented in tiles of 4096 with 1024 overlap
Printed, each the median of --repeats calls after one untimed call (a JSON line per raster):
  wall_ms        outlines.traceSegmentOutlines(labels, maxSegId=...) from the call to the arrays and columns on the host
  device_ms      the library's events round its kernels, and steps_device_ms its split: edges (sides and their scan),
                 successors, rounds (the pointer doubling), rings (leaders, sort, vertices, areas, offsets)
  rounds, edges, rings, vertices, and the longest ring in edges
  shapes_device_ms   shapes.calcSegmentShapes(...).deviceMs on the same labels, for comparison
The untimed call is checked against the shape table: per id the ring areas sum to twice ``area`` and the ring lengths to
``perimeter``, and every id's first ring is an outer ring.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def ring_lengths(o):
    v = o.vertices
    vo = o.vertexOffsets
    nxt = np.arange(len(v)) + 1
    ringOf = np.repeat(np.arange(len(vo) - 1), np.diff(vo))
    last = nxt == vo[1:][ringOf]
    nxt[last] = vo[:-1][ringOf][last]
    cs = np.concatenate([[0], np.cumsum(np.abs(v[nxt] - v).sum(axis=1))])
    return cs[vo[1:]] - cs[vo[:-1]]


def check_against_shapes(o, s):
    ro = o.ringOffsets
    a2 = np.concatenate([[0], np.cumsum(o.ringArea2)])
    assert np.array_equal(a2[ro[1:]] - a2[ro[:-1]], 2 * s.columns['area'])
    lengths = ring_lengths(o)
    ln = np.concatenate([[0], np.cumsum(lengths)])
    assert np.array_equal(ln[ro[1:]] - ln[ro[:-1]], s.columns['perimeter'])
    assert o.edges == int(s.columns['perimeter'].sum())
    has = np.flatnonzero(np.diff(ro) > 0)
    assert np.all(o.ringArea2[ro[has]] > 0)
    return int(lengths.max()) if len(lengths) else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tile-size', type=int, default=4096)
    ap.add_argument('--mosaic-size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--eight', action='store_true')
    ap.add_argument('--skip-tile', action='store_true')
    ap.add_argument('--skip-mosaic', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyshepseg_amd import outlines, shapes, tiling
    out = open(a.out, 'a') if a.out else None

    def measure(what, labels, nrows, ncols, maxSegId):
        (wall, dev, steps) = ([], [], [])
        longest = 0
        for rep in range(-1, a.repeats):
            t = time.perf_counter()
            r = outlines.traceSegmentOutlines(labels, fourConnected=not a.eight, maxSegId=maxSegId)
            if rep >= 0:
                wall.append((time.perf_counter() - t) * 1e3)
                dev.append(r.deviceMs)
                steps.append(r.deviceStepsMs)
            else:
                s = shapes.calcSegmentShapes(labels, maxSegId=maxSegId)
                longest = check_against_shapes(r, s)
        sh = [shapes.calcSegmentShapes(labels, maxSegId=maxSegId).deviceMs for _rep in range(max(2, a.repeats))][1:]
        line = json.dumps(dict(
            what=what, rows=nrows, cols=ncols, runs=len(wall), four_connected=not a.eight, segments=maxSegId,
            wall_ms=round(statistics.median(wall), 1), wall_min_ms=round(min(wall), 1), wall_max_ms=round(max(wall), 1),
            device_ms=round(statistics.median(dev), 2), device_min_ms=round(min(dev), 2), device_max_ms=round(max(dev), 2),
            steps_device_ms={k: round(statistics.median(st[k] for st in steps), 3) for k in steps[0]},
            rounds=r.rounds, edges=r.edges, rings=len(r.ringArea2), vertices=len(r.vertices), longest_ring_edges=longest,
            shapes_device_ms=round(statistics.median(sh), 2), steps_s={k: round(v, 4) for (k, v) in r.timings.items()}))
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


if __name__ == '__main__':
    main()
