"""Convex hulls of the segments on the label raster of one synthetic tile and of a tiled mosaic.

    python tools/perf_hulls.py [--tile-size 4096] [--mosaic-size 16384] [--repeats 3] [--eight] [--skip-tile] [--skip-mosaic] [--out results.jsonl]

The two label rasters of tools/perf_outlines.py, kept in HBM by the segmentation and read in place:
  tile     the labels of --tile-size x --tile-size synthetic 3-band imagery segmented as ONE tile
  mosaic   the labels of --mosaic-size x --mosaic-size imagery segmented in tiles of 4096 with 1024 overlap
Printed, each the median of --repeats calls of outlines.traceSegmentOutlines(labels, maxSegId=..., hulls=True) after one
untimed call (a JSON line per raster):
  hull_device_ms     the library's events round the hull kernels, and hull_steps_device_ms its split: candidates, order
                     (three sorts, the column filter, the ids' ranges), chains, points, reach
  trace_device_ms    the trace's kernels in the same call; hull_over_trace their ratio
  hull_wall_ms       calcSegmentHulls inside that call, from the rings in HBM to the columns on the host, with the
                     download, and hull_steps_s its split; wall_ms the whole call
  vertices, candidates, kept (after the column filter), hull_points
The untimed call is checked against the shape table: hullArea2 >= the id's outer ring areas, at least four hull
points wherever there are pixels, feretMin <= feretMax, 0 < solidity <= 1, feretMax2 >= the squares of the bounding
box's height and width and <= their sum; and every ring vertex of every --check-every-th id lies on or inside its hull,
whose per-edge maximum is the reach.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def check_against_shapes(o, h, s, every):
    (ro, vo, ho) = (o.ringOffsets, o.vertexOffsets, h.hullOffsets)
    has = s.columns['area'] > 0
    outer = np.concatenate([[0], np.cumsum(np.where(o.ringArea2 > 0, o.ringArea2, 0))])
    assert np.all(h.sums['hullArea2'] >= outer[ro[1:]] - outer[ro[:-1]])
    assert np.array_equal(h.sums['numHullVertices'] > 0, has) and np.all(h.sums['numHullVertices'][has] >= 4)
    assert np.all(h.columns['feretMin'][has] <= h.columns['feretMax'][has])
    assert np.all((h.columns['solidity'][has] > 0) & (h.columns['solidity'][has] <= 1))
    height = s.columns['rowMax'] - s.columns['rowMin'] + 1
    width = s.columns['colMax'] - s.columns['colMin'] + 1
    f2 = h.sums['feretMax2']
    assert np.all(f2[has] >= height[has] ** 2) and np.all(f2[has] >= width[has] ** 2) and np.all(f2[has] <= height[has] ** 2 + width[has] ** 2)
    for i in np.flatnonzero(has)[::every].tolist():
        p = h.hullPoints[ho[i]:ho[i + 1]]
        e = np.roll(p, -1, axis=0) - p
        v = o.vertices[vo[ro[i]]:vo[ro[i + 1]]]
        side = e[:, 1][:, None] * (v[:, 0][None, :] - p[:, 0][:, None]) - e[:, 0][:, None] * (v[:, 1][None, :] - p[:, 1][:, None])
        assert side.min() >= 0 and np.array_equal(side.max(axis=1), h.hullReach[ho[i]:ho[i + 1]]), i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tile-size', type=int, default=4096)
    ap.add_argument('--mosaic-size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--eight', action='store_true')
    ap.add_argument('--skip-tile', action='store_true')
    ap.add_argument('--skip-mosaic', action='store_true')
    ap.add_argument('--check-every', type=int, default=97)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyshepseg_amd import outlines, shapes, tiling
    out = open(a.out, 'a') if a.out else None

    def measure(what, labels, nrows, ncols, maxSegId):
        (wall, hwall, dev, tdev, steps) = ([], [], [], [], [])
        for rep in range(-1, a.repeats):
            t = time.perf_counter()
            r = outlines.traceSegmentOutlines(labels, fourConnected=not a.eight, maxSegId=maxSegId, hulls=True)
            if rep >= 0:
                wall.append((time.perf_counter() - t) * 1e3)
                hwall.append(r.timings['hulls'] * 1e3)
                dev.append(r.hulls.deviceMs)
                tdev.append(r.deviceMs)
                steps.append(r.hulls.deviceStepsMs)
                assert not r.hulls.timings['uploaded']
            else:
                check_against_shapes(r, r.hulls, shapes.calcSegmentShapes(labels, maxSegId=maxSegId), a.check_every)
        h = r.hulls
        line = json.dumps(dict(
            what=what, rows=nrows, cols=ncols, runs=len(wall), four_connected=not a.eight, segments=maxSegId,
            hull_device_ms=round(statistics.median(dev), 2), hull_device_min_ms=round(min(dev), 2), hull_device_max_ms=round(max(dev), 2),
            hull_steps_device_ms={k: round(statistics.median(st[k] for st in steps), 3) for k in steps[0]},
            trace_device_ms=round(statistics.median(tdev), 2),
            hull_over_trace=round(statistics.median(dev) / statistics.median(tdev), 3),
            hull_wall_ms=round(statistics.median(hwall), 1), wall_ms=round(statistics.median(wall), 1),
            wall_min_ms=round(min(wall), 1), wall_max_ms=round(max(wall), 1),
            vertices=len(r.vertices), rings=len(r.ringArea2), candidates=h.candidates, kept=h.kept, hull_points=len(h.hullPoints),
            largest_hull=int(h.sums['numHullVertices'].max()), hull_steps_s={k: round(float(v), 4) for (k, v) in h.timings.items()}))
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
