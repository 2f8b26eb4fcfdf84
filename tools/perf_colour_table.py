"""Colour table and rendering at the C5 size: the three mean columns of a 40000 x 40000 raster of 4 x 8-pixel
blocks (50 M segments; the device-side synthetic image and block labels of tools/perf_stats_c5.py).

    python tools/perf_colour_table.py [--size 40000] [--repeats 5] [--skip-numpy] [--out results.jsonl]

Printed, each the median of --repeats runs after one untimed run (a JSON line per figure):
  numpy         the reference's expression (utils.py:216-221: two numpy.percentile and the stretch per column)
                on this host's CPUs with numpy's defaults, three float64 columns
  table_f64     writeColorTableFromRatColumns on the same three pageable float64 columns (what a RAT hands over),
                host columns in to host byte columns out: upload and download included; `device_ms` is the device
                time alone, from the library's events around the kernels of the three columns
  table_f32     the same on the float32 columns as calcPerSegmentStatsTiledBands returns them (converted on the device)
  lookup        the lookup kernel over the label raster resident in HBM into a device buffer, in the renderer's row
                blocks; GB/s counts 4 B read + 4 B gathered + 4 B written per pixel
  render        renderColourTable of the resident labels into a host array (the 4 B per pixel download included)
The byte columns of table_f64 are compared with numpy's before anything is timed."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

BH, BW = 4, 8


def numpy_table(cols):
    out = []
    for col in cols:
        lo = np.percentile(col, 5)
        hi = np.percentile(col, 95)
        out.append((255 * ((col - lo) / (hi - lo)).clip(0, 1)).astype(np.uint8))
    return out


class ResidentLabels(object):
    def __init__(self, ptr, n, S):
        self.outDev = (ptr, n, n, n * n * 4)
        self.maxSegId = S
        self.hist = np.full(S + 1, BH * BW, dtype=np.int64)
        self.hist[0] = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=40000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--skip-numpy', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyshepseg_amd import tiling, tilingstats, utils, _lib
    n = a.size
    if n % BH or n % BW:
        raise SystemExit('--size must be a multiple of %d' % BW)
    c = _lib.ctx()
    L = c._L
    out = open(a.out, 'a') if a.out else None

    def report(what, times, **more):
        line = json.dumps(dict(what=what, rows=S + 1, size=n, runs=len(times), median_ms=round(statistics.median(times), 2),
                               min_ms=round(min(times), 2), max_ms=round(max(times), 2), **more))
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    def timed(fn):
        times = []
        extra = []
        for rep in range(-1, a.repeats):
            t = time.perf_counter()
            r = fn()
            if rep >= 0:
                times.append((time.perf_counter() - t) * 1e3)
                extra.append(r)
        return (times, extra)

    ras = tiling.DeviceRaster.synth(11, 3, n, n)
    d_seg = ctypes.c_void_p()
    c.check(L.shp_dev_alloc(c.handle, n * n * 4, ctypes.byref(d_seg)))
    d_out = ctypes.c_void_p()
    try:
        Sc = ctypes.c_uint32(0)
        c.check(L.shp_dev_block_labels(c.handle, n, n, BH, BW, d_seg, ctypes.byref(Sc)))
        S = Sc.value
        seg = ResidentLabels(d_seg.value, n, S)
        names = ['Band_%d_mean' % b for b in (1, 2, 3)]
        res = tilingstats.calcPerSegmentStatsTiledBands(ras, [(b + 1, [(names[b], 'mean')]) for b in range(3)], seg,
                                                        segSize=seg.hist)
        f32 = {k: res.columns[k] for k in names}
        f64 = {k: res.columns[k].astype(np.float64) for k in names}
        print('%d segments; columns %s' % (S, ', '.join('%s [%.1f, %.1f]' % (k, f64[k][1:].min(), f64[k].max()) for k in names)),
              flush=True)
        table = utils.writeColorTableFromRatColumns(f64, *names)
        if not a.skip_numpy:
            want = numpy_table([f64[k] for k in names])
            for (k, w) in zip(('Red', 'Green', 'Blue'), want):
                if not np.array_equal(table.columns[k], w):
                    raise SystemExit('%s differs from numpy in %d rows' % (k, int((table.columns[k] != w).sum())))
            print('byte columns equal numpy\'s', flush=True)
            (times, _e) = timed(lambda: numpy_table([f64[k] for k in names]))
            report('numpy', times, numpy=np.__version__, cpus=len(os.sched_getaffinity(0)))
        (times, extra) = timed(lambda: utils.writeColorTableFromRatColumns(f64, *names).deviceMs)
        report('table_f64', times, device_ms=round(statistics.median(extra), 3))
        (times, extra) = timed(lambda: utils.writeColorTableFromRatColumns(f32, *names).deviceMs)
        report('table_f32', times, device_ms=round(statistics.median(extra), 3))

        # the lookup kernel alone, in the renderer's row blocks, into a device buffer
        cols = utils._colourColumns(table)
        d_table = ctypes.c_void_p()
        c.check(L.shp_dev_alloc(c.handle, (S + 1) * 4, ctypes.byref(d_table)))
        rows = max(1, tilingstats.STATS_CHUNK_PIXELS // n)
        c.check(L.shp_dev_alloc(c.handle, min(rows, n) * n * 4, ctypes.byref(d_out)))
        c.check(L.shp_colour_pack(c.handle, _lib.ptr(cols[0]), _lib.ptr(cols[1]), _lib.ptr(cols[2]), _lib.ptr(cols[3]),
                                  S + 1, d_table))

        def lookup():
            for y0 in range(0, n, rows):
                y1 = min(n, y0 + rows)
                c.check(L.shp_colour_lookup_dev(c.handle, ctypes.c_void_p(d_seg.value + 4 * y0 * n), (y1 - y0) * n,
                                                d_table, S + 1, d_out))
        (times, _e) = timed(lookup)
        report('lookup', times, gb_per_s=round(12.0 * n * n / 1e9 / (statistics.median(times) / 1e3), 1),
               blocks=len(range(0, n, rows)))
        c.check(L.shp_dev_free(c.handle, d_table))
        (times, _e) = timed(lambda: utils.renderColourTable(seg, table).shape)
        report('render', times, gb_per_s=round(12.0 * n * n / 1e9 / (statistics.median(times) / 1e3), 1))
    finally:
        if d_out.value:
            c.check(L.shp_dev_free(c.handle, d_out))
        c.check(L.shp_dev_free(c.handle, d_seg))
        ras.free()


if __name__ == '__main__':
    main()
