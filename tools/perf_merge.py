"""mergeSegments at the C5 size: the neighbour table of a 40000 x 40000 raster of 4 x 8-pixel blocks (50 M segments,
the device-side block labels of tools/perf_stats_c5.py), merged under the key column id % 5, step by step.

    python tools/perf_merge.py [--size 40000] [--repeats 3] [--out results.jsonl]

A row of the raster holds size / 8 blocks; where that is a multiple of 5 (40000: 5000) a block and the block below it
share their key, so every COLUMN of blocks becomes one group: size / 8 groups of size / 4 segments each, hooked along
chains of that length -- far more merging than a classification gives.

Printed, each the median of --repeats calls after one untimed call (one JSON line):
  hook / renumber / contract / recode _ms   the library's device events around the kernels of the step
  *_gb and *_hbm_fraction                   the bytes the step must move (below) and that over the device time as a
                                            fraction of 8 TB/s
  wall_ms, upload_ms                        mergeSegments from the call to its result; of that the upload of the old
                                            table, which the contracted one displaced in the call before
  recode_count_ms                           the raster pass when it also counts the new histogram (no segSize)
  lookup_ms                                 shp_colour_lookup_dev over the same raster with the recode as its table, in the
                                            same row blocks (wall time around the synchronous calls)
Bytes: hook = the table (8 B per row, 12 B per entry) + two gathered 8-byte keys and sizes per entry a < b; renumber =
40 B per row (parent in, root out; root, size in, index out; root, index, size in, recode out); contract = the table + 8 B
of gathered recodes per entry a < b + 16 B per record out, and the sort's passes over the records, which are not counted;
recode = 4 B in, 4 B gathered, 4 B out per pixel.
Checked before anything is timed: the groups' sizes and histogram add up, every representative recodes to its own group,
and findSegmentNeighbours of the recoded raster gives the contracted table array for array."""
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
    def __init__(self, ptr, n):
        self.outDev = (ptr, n, n, n * n * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=40000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyshepseg_amd import neighbours, tiling, tilingstats, _lib
    n = a.size
    if n % BH or n % BW:
        raise SystemExit('--size must be a multiple of %d' % BW)
    c = _lib.ctx()
    L = c._L
    d_seg = ctypes.c_void_p()
    c.check(L.shp_dev_alloc(c.handle, n * n * 4, ctypes.byref(d_seg)))
    (d_table, d_out) = (ctypes.c_void_p(), ctypes.c_void_p())
    try:
        Sc = ctypes.c_uint32(0)
        c.check(L.shp_dev_block_labels(c.handle, n, n, BH, BW, d_seg, ctypes.byref(Sc)))
        S = Sc.value
        seg = ResidentLabels(d_seg.value, n)
        t = time.perf_counter()
        nb = neighbours.findSegmentNeighbours(seg, True, maxSegId=S)
        print('%d segments, %d entries; table in %.2f s (%.1f ms on the device)' % (
            S, len(nb.neighbours), time.perf_counter() - t, nb.deviceMs), flush=True)
        keys = np.arange(S + 1, dtype=np.int64) % 5
        size = np.full(S + 1, BH * BW, dtype=np.int64)
        size[0] = 0

        # ---- the result, checked once ----
        res = neighbours.mergeSegments(nb, keys, segSize=size, segfile=seg)
        M = res.maxSegId
        assert res.groupSize.sum() == S and res.hist.sum() == n * n and res.hist[0] == 0
        assert np.array_equal(res.recode[res.representative[1:]], np.arange(1, M + 1))
        again = neighbours.findSegmentNeighbours(res, True, maxSegId=M)
        for name in ('offsets', 'neighbours', 'borderLengths'):
            assert np.array_equal(getattr(again, name), getattr(res.neighbours, name)), name
        half = len(nb.neighbours) // 2
        print('%d groups, %d links, %d records, %d entries; the recoded raster gives the same table' % (
            M, res.links, res.recordsSorted, len(res.neighbours.neighbours)), flush=True)
        (records, entriesOut) = (res.recordsSorted, len(res.neighbours.neighbours))
        recode = res.recode
        tiling.freeDeviceOutput(res)
        del again

        steps = {k: [] for k in ('hook', 'renumber', 'contract', 'recode')}
        (wall, upload, count) = ([], [], [])
        for rep in range(a.repeats):
            t = time.perf_counter()
            res = neighbours.mergeSegments(nb, keys, segSize=size, segfile=seg)
            wall.append((time.perf_counter() - t) * 1e3)
            assert res.timings['uploaded']
            upload.append(res.timings['upload'] * 1e3)
            for k in steps:
                steps[k].append(res.stepDeviceMs[k])
            tiling.freeDeviceOutput(res)
            res = neighbours.mergeSegments(nb, keys, segfile=seg)
            count.append(res.stepDeviceMs['recode'])
            assert res.hist.sum() == n * n
            tiling.freeDeviceOutput(res)

        # ---- the colour lookup over the same raster, the recode as its table ----
        rows = max(1, tilingstats.STATS_CHUNK_PIXELS // n)
        c.check(L.shp_dev_alloc(c.handle, (S + 1) * 4, ctypes.byref(d_table)))
        c.check(L.shp_dev_alloc(c.handle, min(rows, n) * n * 4, ctypes.byref(d_out)))
        c.check(L.shp_dev_upload(c.handle, d_table, _lib.ptr(recode), recode.nbytes))
        lookup = []
        for rep in range(-1, a.repeats):
            t = time.perf_counter()
            for y0 in range(0, n, rows):
                y1 = min(n, y0 + rows)
                c.check(L.shp_colour_lookup_dev(c.handle, ctypes.c_void_p(d_seg.value + 4 * y0 * n), (y1 - y0) * n,
                                                d_table, S + 1, d_out))
            if rep >= 0:
                lookup.append((time.perf_counter() - t) * 1e3)

        table = 8.0 * (S + 2) + 12.0 * len(nb.neighbours)
        gb = {'hook': table + 32.0 * half, 'renumber': 40.0 * (S + 1),
              'contract': table + 8.0 * half + 16.0 * records + 8.0 * (M + 2) + 12.0 * entriesOut,
              'recode': 12.0 * n * n}
        line = dict(size=n, segments=S, entries=len(nb.neighbours), groups=M, links=res.links, records=records,
                    runs=a.repeats, wall_ms=round(statistics.median(wall), 1), upload_ms=round(statistics.median(upload), 1),
                    recode_count_ms=round(statistics.median(count), 3), lookup_ms=round(statistics.median(lookup), 3),
                    lookup_blocks=len(range(0, n, rows)))
        for k in steps:
            ms = statistics.median(steps[k])
            line[k + '_ms'] = round(ms, 3)
            line[k + '_min_max_ms'] = [round(min(steps[k]), 3), round(max(steps[k]), 3)]
            line[k + '_gb'] = round(gb[k] / 1e9, 3)
            line[k + '_hbm_fraction'] = round(gb[k] / HBM_PEAK / (ms / 1e3), 4)
        line = json.dumps(line)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    finally:
        for p in (d_table, d_out, d_seg):
            if p.value:
                c.check(L.shp_dev_free(c.handle, p))


if __name__ == '__main__':
    main()
