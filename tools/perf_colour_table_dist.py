"""Colour table and RGBA rendering on the row-sharded multi-rank output, at the benchmark raster's size: a
device-resident N x N raster of 4 x 8-pixel block labels (N = 40000: 50 M segments, the labels of
tools/perf_colour_table.py) and three float32 columns of N * N / 32 + 1 rows.

    python tools/perf_colour_table_dist.py [--size 40000] [--worlds 1,2,4] [--repeats 3] [--scratch DIR] [--skip-parent]

Printed as JSON lines (each the median of --repeats runs after one untimed run):
  parent_table    what the commit before could do for the same table: utils.writeColorTableFromRatColumns of the
                  whole columns in one process on one GPU (wall and device ms)
  parent_render   utils.renderColourTable of the label raster written to a .npy file in --scratch into an RGBA
                  .npy file there, in one process (the labels are written by this script, untimed)
  dist_table      distributed.deviceColourTable with W rank threads that SHARE this one GPU (every rank a context
                  of its own, device collectives as device copies: tests/stats_bands_dist_helpers.ThreadDevComm):
                  per rank wall ms and device ms of its share, rows, and the exchanged bytes of the job.  The
                  ranks' kernels run side by side on one GPU here, so the per-rank device time is an upper bound of
                  what a rank with a GPU of its own spends; the tables are compared with the parent's
  dist_render     distributed.deviceRender of every rank's rows, the ranks one after the other (a rank's render
                  has no collective but the closing all-gather of the errors): per rank wall ms, the summed lookup
                  and download device times and the wall time of the render calls -- `overlap_pays` when that wall
                  time is below lookup + download --, and GB/s of pixels delivered to the host (4 B each)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
BH, BW = 4, 8


class OneRank(object):
    """the collectives of a rank that renders alone"""
    (rank, world) = (0, 1)

    def allgather_obj(self, obj):
        return [obj]


def median(v):
    return round(statistics.median(v), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=40000)
    ap.add_argument('--worlds', default='1,2,4')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--scratch', default=os.environ.get('SHEPSEG_SCRATCH', '/tmp'))
    ap.add_argument('--skip-parent', action='store_true')
    a = ap.parse_args()
    from pyshepseg_amd import distributed, tiling, utils, _lib
    import stats_bands_dist_helpers as H
    n = a.size
    if n % BH or n % BW:
        raise SystemExit('--size must be a multiple of %d' % BW)
    c = _lib.ctx()
    L = c._L
    d_seg = ctypes.c_void_p()
    c.check(L.shp_dev_alloc(c.handle, n * n * 4, ctypes.byref(d_seg)))
    Sc = ctypes.c_uint32(0)
    c.check(L.shp_dev_block_labels(c.handle, n, n, BH, BW, d_seg, ctypes.byref(Sc)))
    S = Sc.value
    rng = np.random.default_rng(1)
    names = ['mean1', 'mean2', 'mean3']
    cols = {k: (rng.normal(900.0 + 300.0 * i, 250.0, size=S + 1)).astype(np.float32) for (i, k) in enumerate(names)}

    def report(what, **more):
        print(json.dumps(dict(what=what, size=n, rows=S + 1, **more)), flush=True)

    def timed(fn):
        (times, extra) = ([], [])
        for rep in range(-1, a.repeats):
            t = time.perf_counter()
            r = fn()
            if rep >= 0:
                times.append((time.perf_counter() - t) * 1e3)
                extra.append(r)
        return times, extra

    table = utils.writeColorTableFromRatColumns(cols, *names)
    try:
        if not a.skip_parent:
            (times, extra) = timed(lambda: utils.writeColorTableFromRatColumns(cols, *names).deviceMs)
            report('parent_table', wall_ms=median(times), device_ms=median(extra))
            labels = os.path.join(a.scratch, 'perf_colour_labels_%d.npy' % os.getpid())
            rgba = os.path.join(a.scratch, 'perf_colour_rgba_%d.npy' % os.getpid())
            try:
                w = tiling._NpyRowWriter(labels, n, n)
                rows = max(1, (256 << 20) // (4 * n))
                buf = np.empty((rows, n), dtype=np.uint32)
                for y in range(0, n, rows):
                    y1 = min(n, y + rows)
                    c.check(L.shp_dev_download(c.handle, _lib.ptr(buf), ctypes.c_void_p(d_seg.value + 4 * y * n),
                                               (y1 - y) * n * 4))
                    w.writeRows(y, y1, buf[:y1 - y])
                w.close()
                (times, _e) = timed(lambda: utils.renderColourTable(labels, table, outfile=rgba))
                report('parent_render', wall_ms=median(times), gb_per_s=round(4.0 * n * n / 1e6 / median(times), 2))
            finally:
                for p in (labels, rgba):
                    if os.path.exists(p):
                        os.remove(p)
        packed = np.stack([table.columns[k] for k in utils.COLOUR_NAMES], -1).view(np.uint32).ravel()
        for W in [int(v) for v in a.worlds.split(',')]:
            # ---- the table: W rank threads on this GPU
            def body(r, comm, pc):
                walls, devs = [], []
                for rep in range(-1, a.repeats):
                    info = {}
                    comm.allgather_obj(None)                        # the ranks start together
                    t = time.perf_counter()
                    (columns, stretch, ms, d_table, rowsN) = distributed.deviceColourTable(pc, comm, [cols[k] for k in names],
                                                                                          info=info)
                    wall = (time.perf_counter() - t) * 1e3
                    got = np.empty(rowsN, dtype=np.uint32)
                    pc.check(L.shp_dev_download(pc.handle, _lib.ptr(got), d_table, got.nbytes))
                    tiling._devRelease(pc, d_table, rowsN * 4)
                    if not np.array_equal(got, packed) or stretch != table.stretch:
                        raise SystemExit('rank %d of %d: the table differs from the one-GPU table' % (r, W))
                    if rep >= 0:
                        walls.append(wall)
                        devs.append(ms)
                return dict(rank=r, rows=info['rows'][1] - info['rows'][0], wall_ms=median(walls), device_ms=median(devs),
                            exchange_bytes=info['exchange_bytes'])
            (results, errors) = H.runRankThreads(W, body, timeout=1800)
            if any(errors):
                raise SystemExit('world %d: %s' % (W, errors))
            report('dist_table', world=W, ranks=results, exchange_bytes=results[0]['exchange_bytes'],
                   max_wall_ms=max(q['wall_ms'] for q in results))
            # ---- the render: every rank's rows, one rank at a time
            cuts = [r * n // W for r in range(W)] + [n]
            d_table = tiling._devAlloc(c, (S + 1) * 4)
            c.check(L.shp_dev_upload(c.handle, d_table, _lib.ptr(packed), packed.nbytes))
            ranks = []
            try:
                for r in range(W):
                    (lo, hi) = (cuts[r], cuts[r + 1])
                    infos = []

                    def render():
                        info = {}
                        distributed.deviceRender(c, OneRank(), d_seg.value + 4 * lo * n, hi - lo, n, d_table, S + 1,
                                                 sink=lambda y0, y1, rows: None, info=info)
                        infos.append(info)
                    (times, _e) = timed(render)
                    infos = infos[1:]
                    q = dict(rank=r, rows=hi - lo, wall_ms=median(times), blocks=infos[0]['blocks'],
                             lookup_ms=median([i['lookupMs'] for i in infos]),
                             download_ms=median([i['downloadMs'] for i in infos]),
                             render_ms=median([i['renderMs'] for i in infos]))
                    q['overlap_pays'] = bool(q['render_ms'] < q['lookup_ms'] + q['download_ms'])
                    q['gb_per_s'] = round(4.0 * (hi - lo) * n / 1e6 / q['render_ms'], 2)
                    ranks.append(q)
            finally:
                tiling._devRelease(c, d_table, (S + 1) * 4)
            report('dist_render', world=W, ranks=ranks, max_wall_ms=max(q['wall_ms'] for q in ranks))
    finally:
        c.check(L.shp_dev_free(c.handle, d_seg))


if __name__ == '__main__':
    main()
