"""The junction trace and the simplification of the rings on the label rasters of the hull table and on random labels.

    python tools/perf_simplify.py [--tile-size 4096] [--mosaic-size 16384] [--repeats 3] [--eight] [--skip-tile] [--skip-mosaic] [--skip-random] [--out results.jsonl]

The label rasters of tools/perf_hulls.py, kept in HBM by the segmentation and read in place, and a host raster:
  tile        the labels of --tile-size x --tile-size synthetic 3-band imagery segmented as ONE tile
  mosaic      the labels of --mosaic-size x --mosaic-size imagery segmented in tiles of 4096 with 1024 overlap
  random1024  1024 x 1024 labels drawn per pixel from 40 000 ids (arcs of two and three points), uploaded by every trace
Printed, each the median of --repeats calls after one untimed call (a JSON line per raster):
  plain_trace_device_ms      outlines.traceSegmentOutlines(labels, maxSegId=...), the library's events round its kernels,
                             with the smallest and the largest call
  junction_trace_device_ms   the same with junctions=True, in the same process, in turns with the plain trace;
                             junction_over_plain their ratio; vertices and junction_vertices, plain_vertices
  per tolerance 0.5, 1, 1.5  outlines.simplifySegmentOutlines of the resident junction trace: device_ms and steps_device_ms
                             (arcs, rounds, areas, emit), wall_ms with the download, arcs, their classes, longest_arc, rounds,
                             vertices_after, rings_after, dropped_rings
The untimed calls are checked: the junction trace has the plain trace's ring areas, every junction vertex is kept, the
result's vertices are the source's kept ones, and the plain trace after the junction trace returns the bytes it returned
before.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

TOLERANCES = (0.5, 1.0, 1.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tile-size', type=int, default=4096)
    ap.add_argument('--mosaic-size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--eight', action='store_true')
    ap.add_argument('--skip-tile', action='store_true')
    ap.add_argument('--skip-mosaic', action='store_true')
    ap.add_argument('--skip-random', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyshepseg_amd import outlines, tiling
    out = open(a.out, 'a') if a.out else None

    def measure(what, labels, nrows, ncols, maxSegId):
        (plain, junc) = ([], [])
        first = None
        for rep in range(-1, a.repeats):
            p = outlines.traceSegmentOutlines(labels, fourConnected=not a.eight, maxSegId=maxSegId)
            o = outlines.traceSegmentOutlines(labels, fourConnected=not a.eight, maxSegId=maxSegId, junctions=True)
            if rep >= 0:
                plain.append(p.deviceMs)
                junc.append(o.deviceMs)
            else:
                first = p
                assert np.array_equal(o.ringArea2, p.ringArea2) and np.array_equal(o.ringOffsets, p.ringOffsets)
        again = outlines.traceSegmentOutlines(labels, fourConnected=not a.eight, maxSegId=maxSegId)
        for k in ('ringOffsets', 'vertexOffsets', 'vertices', 'ringArea2'):
            assert getattr(again, k).tobytes() == getattr(first, k).tobytes(), k
        plain_vertices = len(again.vertices)
        del again, first, p
        o = outlines.traceSegmentOutlines(labels, fourConnected=not a.eight, maxSegId=maxSegId, junctions=True)
        per = {}
        for tol in TOLERANCES:
            (dev, wall, steps) = ([], [], [])
            for rep in range(-1, a.repeats):
                t = time.perf_counter()
                s = outlines.simplifySegmentOutlines(o, tol)
                if rep >= 0:
                    wall.append((time.perf_counter() - t) * 1e3)
                    dev.append(s.deviceMs)
                    steps.append(s.deviceStepsMs)
                    assert not s.timings['uploaded']
                else:
                    kept = np.zeros(len(o.vertices), dtype=bool)
                    kept[s.keptVertex] = True
                    alive = np.zeros(len(o.ringArea2), dtype=bool)
                    alive[s.sourceRing] = True
                    inring = np.repeat(alive, np.diff(o.vertexOffsets))
                    assert np.all(kept[(o.junction == 1) & inring]) and np.array_equal(s.vertices, o.vertices[s.keptVertex])
            per[str(tol)] = dict(
                device_ms=round(statistics.median(dev), 2), device_min_ms=round(min(dev), 2), device_max_ms=round(max(dev), 2),
                steps_device_ms={k: round(statistics.median(st[k] for st in steps), 3) for k in steps[0]},
                wall_ms=round(statistics.median(wall), 1), arcs=s.arcs, arc_classes=s.arcClasses, longest_arc=s.longestArc,
                rounds=s.rounds, vertices_after=len(s.vertices), rings_after=len(s.ringArea2), dropped_rings=int(s.droppedRings.sum()))
        line = json.dumps(dict(
            what=what, rows=nrows, cols=ncols, runs=len(plain), four_connected=not a.eight, segments=maxSegId,
            plain_trace_device_ms=round(statistics.median(plain), 2), plain_trace_device_min_ms=round(min(plain), 2),
            plain_trace_device_max_ms=round(max(plain), 2), junction_trace_device_ms=round(statistics.median(junc), 2),
            junction_trace_device_min_ms=round(min(junc), 2), junction_trace_device_max_ms=round(max(junc), 2),
            junction_over_plain=round(statistics.median(junc) / statistics.median(plain), 3), plain_vertices=plain_vertices,
            vertices=len(o.vertices), junction_vertices=int(o.junction.sum()), rings=len(o.ringArea2), simplify=per))
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
    if not a.skip_random:
        rng = np.random.default_rng(1)
        seg = rng.integers(1, 40000, size=(1024, 1024), dtype=np.uint32)
        measure('random1024', seg, 1024, 1024, 39999)


if __name__ == '__main__':
    main()
