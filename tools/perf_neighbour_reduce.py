"""Columns reduced over the neighbour table: neighbours.reduceOverNeighbours against its numpy expression.

    python tools/perf_neighbour_reduce.py [--seg-size 8192] [--rows 50000000] [--repeats 3] [--skip-seg] [--skip-synth]
                                          [--skip-host] [--out results.jsonl]

Two tables, a float64 column uniform in (-1000, 1000), all nine statistics:
  segment  the table of the labels a tiled segmentation of --seg-size x --seg-size synthetic 3-band imagery keeps on
           the device, built by findSegmentNeighbours just before: RESIDENT, nothing is uploaded
  synth    --rows rows of geometric degrees (mean 6) and five rows of 10^5 .. 10^6 entries, built with numpy (not
           symmetric, valid): UPLOADED by the first call and checked on the device, resident in the calls after it
Printed, each the median of --repeats calls after the first (a JSON line per table):
  device_ms      the library's events around the kernels of the call (no transfers)
  wall_ms        reduceOverNeighbours from the call to the nine host columns; upload_ms: the table's upload and check
                 in the first call; column_ms: wall_ms - device_ms, the column's upload and the download of nine
  hbm_fraction   (the table's bytes + 8 B per gathered value) / device_ms as a fraction of 8 TB/s
  host_ms        the numpy expression of the same nine statistics (reduceat over fancy-indexed gathers, plain float64
                 sums: the model of tests/neighbour_reduce_cases.py without its exact summation), one run
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HBM_PEAK = 8.0e12
STATS = ('count', 'border', 'min', 'max', 'mean', 'bordermean', 'meanabsdiff', 'bordertohigher', 'nearest')


def host_expression(offsets, nbrs, lens, v, missing=-9999.0):
    """the nine statistics with numpy on the host; only NaN is ignored"""
    nrows = len(offsets) - 1
    x = v[nbrs]
    keep = ~np.isnan(x)
    row = np.repeat(np.arange(nrows, dtype=np.int64), np.diff(offsets))[keep]
    (x, n, w) = (x[keep], nbrs[keep].astype(np.int64), lens[keep])
    count = np.bincount(row, minlength=nrows)
    rows = np.flatnonzero(count)
    first = (np.cumsum(count) - count)[rows]
    own = v[row]
    own_ok = ~np.isnan(v)

    def per_row(ufunc, values, dtype, fill):
        out = np.full(nrows, fill, dtype=dtype)
        if len(rows):
            out[rows] = ufunc.reduceat(values, first)
        return out
    wf = w.astype(np.float64)
    border = per_row(np.add, w, np.int64, 0)
    d = np.abs(x - own)
    res = {'count': count, 'border': border, 'min': per_row(np.minimum, x, np.float64, missing),
           'max': per_row(np.maximum, x, np.float64, missing)}
    with np.errstate(invalid='ignore', divide='ignore'):
        have = count > 0
        res['mean'] = np.where(have, per_row(np.add, x, np.float64, 0) / count, missing)
        res['bordermean'] = np.where(have, per_row(np.add, wf * x, np.float64, 0) / border, missing)
        res['meanabsdiff'] = np.where(have & own_ok, per_row(np.add, wf * d, np.float64, 0) / border, missing)
    res['bordertohigher'] = np.where(own_ok, per_row(np.add, np.where(x > own, w, 0), np.int64, 0), 0)
    dmin = per_row(np.minimum, d, np.float64, 0)
    big = np.int64(1) << np.int64(40)
    near = per_row(np.minimum, np.where(d == dmin[row], n, big), np.int64, 0)
    res['nearest'] = np.where(have & own_ok & (near < big), near, 0)
    return res


def synthetic_table(nrows, seed=1):
    """offsets, ids, lengths of nrows rows (row 0 empty): geometric degrees of mean 6 (at most 64), ascending ids near
    the row (within about +-2^15, as the ids of a raster's segments are), and as the last five rows long ones of
    10^5 .. 10^6 entries spread over the whole table.  Not symmetric; it keeps the rules of shp_nbr_upload."""
    rng = np.random.default_rng(seed)
    long_deg = np.minimum(np.array([100000, 200000, 400000, 700000, 1000000], dtype=np.int64), max(1, nrows // 4))
    nshort = nrows - len(long_deg)
    deg = np.minimum(rng.geometric(1.0 / 7.0, size=nshort).astype(np.int64) - 1, 64)
    deg[0] = 0
    starts = np.cumsum(deg) - deg
    total = int(deg.sum())
    row = np.repeat(np.arange(nshort, dtype=np.int64), deg)
    # ascending ids: from below the row in steps of 1 + a random gap; the row itself is stepped over
    gap = rng.integers(1, (1 << 10) + 1, size=total, dtype=np.int64)
    run = np.cumsum(gap)
    has = deg > 0
    run -= np.repeat(run[starts[has]] - gap[starts[has]], deg[has])
    ids = row - (1 << 15) + run
    ids += (ids >= row)
    # rows that reach past either end of the table lose their entries
    bad = np.zeros(nshort, dtype=bool)
    bad[row[(ids < 1) | (ids >= nrows)]] = True
    keep = ~bad[row]
    ids = ids[keep]
    deg[bad] = 0
    parts = [ids.astype(np.uint32)]
    for (k, d) in enumerate(long_deg):
        r = nshort + k
        pick = np.sort(rng.choice(nrows - 2, size=int(d), replace=False)) + 1
        pick[pick >= r] += 1
        parts.append(pick.astype(np.uint32))
    deg = np.concatenate([deg, long_deg])
    offsets = np.zeros(nrows + 1, dtype=np.int64)
    np.cumsum(deg, out=offsets[1:])
    ids = np.concatenate(parts)
    lens = rng.integers(1, (1 << 10) + 1, size=len(ids), dtype=np.int64)
    return (offsets, ids, lens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seg-size', type=int, default=8192)
    ap.add_argument('--rows', type=int, default=50000000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--skip-seg', action='store_true')
    ap.add_argument('--skip-synth', action='store_true')
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyshepseg_amd import neighbours, tiling
    out = open(a.out, 'a') if a.out else None

    def measure(what, nb, resident):
        nrows = nb.maxSegId + 1
        col = np.random.default_rng(2).uniform(-1000.0, 1000.0, size=nrows)
        sel = [(col, [(s, s) for s in STATS])]
        (wall, dev) = ([], [])
        first = None
        for rep in range(-1, a.repeats):
            t = time.perf_counter()
            got = neighbours.reduceOverNeighbours(nb, sel)
            ms = (time.perf_counter() - t) * 1e3
            if rep < 0:
                first = dict(nb.reduceTimings, wall_ms=ms)
                assert first['uploaded'] is (not resident)
            else:
                assert not nb.reduceTimings['uploaded']
                wall.append(ms)
                dev.append(nb.reduceTimings['deviceMs'])
        host_ms = None
        if not a.skip_host:
            t = time.perf_counter()
            want = host_expression(nb.offsets, nb.neighbours, nb.borderLengths, col)
            host_ms = (time.perf_counter() - t) * 1e3
            for s in ('count', 'border', 'min', 'max', 'bordertohigher', 'nearest'):
                assert np.array_equal(got[s], want[s]), s
            for s in ('mean', 'bordermean', 'meanabsdiff'):
                assert np.allclose(got[s], want[s], rtol=1e-9, atol=1e-9), s
        entries = len(nb.neighbours)
        table_bytes = 8 * (nrows + 1) + 12 * entries
        ms = statistics.median(dev)
        line = json.dumps(dict(
            what=what, rows=nrows, entries=entries, resident=resident, runs=len(wall),
            max_degree=int(np.diff(nb.offsets).max()) if nrows else 0,
            device_ms=round(ms, 3), device_min_ms=round(min(dev), 3), device_max_ms=round(max(dev), 3),
            wall_ms=round(statistics.median(wall), 1), column_ms=round(statistics.median(wall) - ms, 1),
            first_call_wall_ms=round(first['wall_ms'], 1), upload_ms=round(first['upload'] * 1e3, 1),
            first_call_device_ms=round(first['deviceMs'], 3),
            hbm_fraction=round(((table_bytes + 8.0 * entries) / HBM_PEAK) / (ms / 1e3), 4),
            host_ms=None if host_ms is None else round(host_ms, 1)))
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    if not a.skip_seg:
        m = a.seg_size
        ras = tiling.DeviceRaster.synth(3, 3, m, m)
        try:
            cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=4)
            rd = tiling.doTiledShepherdSegmentation(ras, tiling._KEEP_ON_DEVICE, tileSize=4096, overlapSize=1024,
                                                    minSegmentSize=50, numClusters=60, fixedKMeansInit=True,
                                                    concurrencyCfg=cfg)
            try:
                nb = neighbours.findSegmentNeighbours(rd, fourConnected=True)
            finally:
                tiling.freeDeviceOutput(rd)
        finally:
            ras.free()
        print('segmentation: %d segments, %d entries' % (nb.maxSegId, len(nb.neighbours)), flush=True)
        measure('segment', nb, True)
    if not a.skip_synth:
        t = time.perf_counter()
        (offsets, ids, lens) = synthetic_table(a.rows)
        print('synthetic table: %d rows, %d entries, built in %.1f s' % (a.rows, len(ids), time.perf_counter() - t), flush=True)
        measure('synth', neighbours.SegmentNeighbours(offsets, ids, lens, a.rows - 1, True), False)


if __name__ == '__main__':
    main()
