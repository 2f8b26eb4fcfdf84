"""Per-segment statistics of N bands of a C5-like raster (the device-side synthetic image and the 4 x 8-pixel
block labels of tools/perf_stats_c5.py): ONE call of calcPerSegmentStatsTiledBands against N calls of
calcPerSegmentStatsTiled, (a) with the rasters resident in HBM and (b) from .npy files.

    python tools/perf_stats_bands.py [--variant bands,single] [--bands 1,3,6,10] [--size 40000]
           [--file-size 12000] [--repeats 5] [--dir DIR] [--root REPO] [--out results.jsonl]
    python tools/perf_stats_bands.py --summarise results.jsonl [more.jsonl ...]

Every (variant, N, source) is run once untimed (code objects, workspace growth, page cache) and then --repeats
times; a line of JSON per timed run: wall = host clock around the call(s), which end in a device
synchronisation (the column download); dev = the library's PROF_SEGSTATS event counter over the same call(s).
--root imports pyshepseg_amd from another checkout (a build without calcPerSegmentStatsTiledBands runs
--variant single only): baseline and candidate are then two processes over the same inputs, to be alternated.
--summarise prints min / median / max per (variant, N, source) and the ratio of the medians.
The .npy inputs are written under --dir (default: the system's temporary directory), reused by a later run
that finds them, and their size is printed; nothing outside the repository is read."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

BH, BW = 4, 8
SEL = [('mean', 'mean'), ('sd', 'stddev'), ('med', 'median'), ('n', 'pixcount')]
PROF_SEGSTATS = 8


def summarise(paths):
    rows = {}
    for p in paths:
        for line in open(p):
            if line.startswith('{'):
                r = json.loads(line)
                rows.setdefault((r['n'], r['source'], r['variant'], r.get('tag', '')), []).append(r)
    print('%3s %-8s %-7s %-10s %4s  %-30s %-30s' % ('N', 'source', 'variant', 'tag', 'runs', 'wall ms min/median/max',
                                                   'device ms min/median/max'))
    med = {}
    for key in sorted(rows):
        w = sorted(r['wall_ms'] for r in rows[key])
        d = sorted(r['dev_ms'] for r in rows[key])
        med[key] = (statistics.median(w), statistics.median(d), w[-1] - w[0], d[-1] - d[0])
        print('%3d %-8s %-7s %-10s %4d  %-30s %-30s' % (key + (len(w),
              '%.1f / %.1f / %.1f' % (w[0], med[key][0], w[-1]), '%.2f / %.2f / %.2f' % (d[0], med[key][1], d[-1]))))
    for key in sorted(med):
        if key[2] != 'bands':
            continue
        for other in sorted(med):
            if other[:2] == key[:2] and other[2] == 'single':
                print('N=%d %s: bands[%s] / single[%s]  wall %.3f (spread of single %.1f ms)  device %.3f (spread of single %.2f ms)'
                      % (key[0], key[1], key[3], other[3], med[key][0] / med[other][0], med[other][2],
                         med[key][1] / med[other][1], med[other][3]))


class ResidentLabels(object):
    """what calcPerSegmentStatsTiled expects of a segmentation kept on the device"""
    def __init__(self, ptr, n, S):
        self.outDev = (ptr, n, n, n * n * 4)
        self.maxSegId = S
        self.hist = np.full(S + 1, BH * BW, dtype=np.int64)
        self.hist[0] = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', default='bands,single')
    ap.add_argument('--bands', default='1,3,6,10')
    ap.add_argument('--sources', default='resident,npy')
    ap.add_argument('--size', type=int, default=40000)
    ap.add_argument('--file-size', type=int, default=12000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--dir', default=None)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default=None)
    ap.add_argument('--summarise', nargs='+')
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    sys.path.insert(0, a.root)
    from pyshepseg_amd import tiling, tilingstats, _lib
    variants = a.variant.split(',')
    if 'bands' in variants and not hasattr(tilingstats, 'calcPerSegmentStatsTiledBands'):
        raise SystemExit('%s has no calcPerSegmentStatsTiledBands: run it with --variant single' % a.root)
    counts = [int(x) for x in a.bands.split(',')]
    nbMax = max(counts)
    c = _lib.ctx()
    out = open(a.out, 'a') if a.out else None

    def labels(n):
        if n % BH or n % BW:
            raise SystemExit('sizes must be multiples of %d' % BW)
        d = ctypes.c_void_p()
        c.check(c._L.shp_dev_alloc(c.handle, n * n * 4, ctypes.byref(d)))
        S = ctypes.c_uint32(0)
        c.check(c._L.shp_dev_block_labels(c.handle, n, n, BH, BW, d, ctypes.byref(S)))
        return d, S.value

    def dev_ms(reset):
        ms = (ctypes.c_double * 16)()
        cn = (ctypes.c_uint64 * 16)()
        c.check(c._L.shp_prof_get(c.handle, ms, cn, 16, int(reset)))
        return ms[PROF_SEGSTATS]

    def bandsel(nb):
        return [(b + 1, [('b%d_%s' % (b + 1, s[0]),) + s[1:] for s in SEL]) for b in range(nb)]

    def run(variant, nb, img, seg, hist):
        if variant == 'bands':
            r = tilingstats.calcPerSegmentStatsTiledBands(img, bandsel(nb), seg, segSize=hist)
            return int(r.columns['b%d_n' % nb].sum())
        for (b, sel) in bandsel(nb):
            r = tilingstats.calcPerSegmentStatsTiled(img, b, seg, sel, segSize=hist)
        return int(r.columns['b%d_n' % nb].sum())

    def measure(source, n, img, seg, hist):
        for nb in counts:
            for variant in variants:
                for rep in range(-1, a.repeats):                    # (-1: the untimed run)
                    dev_ms(True)
                    t = time.perf_counter()
                    npx = run(variant, nb, img, seg, hist)
                    wall = (time.perf_counter() - t) * 1e3
                    dev = dev_ms(True)
                    assert npx == n * n, (npx, n * n)
                    if rep < 0:
                        continue
                    line = json.dumps(dict(variant=variant, n=nb, source=source, size=n, rep=rep, tag=a.tag,
                                           wall_ms=round(wall, 2), dev_ms=round(dev, 3)))
                    print(line, flush=True)
                    if out:
                        out.write(line + '\n')
                        out.flush()

    for source in a.sources.split(','):
        n = a.size if source == 'resident' else a.file_size
        if source == 'resident':
            ras = tiling.DeviceRaster.synth(11, nbMax, n, n)
            (d_seg, S) = labels(n)
            try:
                print('resident: %d bands of %d x %d uint16 + labels, %d segments, %.1f GB of HBM'
                      % (nbMax, n, n, S, (nbMax * 2 + 4) * n * n / 1e9), flush=True)
                seg = ResidentLabels(d_seg.value, n, S)
                measure(source, n, ras, seg, seg.hist)
            finally:
                c.check(c._L.shp_dev_free(c.handle, d_seg))
                ras.free()
        else:
            d = a.dir or tempfile.gettempdir()
            ip = os.path.join(d, 'perf_stats_bands_img_%d_%d.npy' % (nbMax, n))
            sp = os.path.join(d, 'perf_stats_bands_seg_%d.npy' % n)
            S = (n // BH) * (n // BW)
            if not (os.path.exists(ip) and os.path.exists(sp)):
                ras = tiling.DeviceRaster.synth(11, nbMax, n, n)
                np.save(ip, ras.toArray())
                ras.free()
                lab = ((np.arange(n, dtype=np.uint32) // BH)[:, None] * np.uint32(n // BW) +
                       (np.arange(n, dtype=np.uint32) // BW)[None, :] + np.uint32(1))
                np.save(sp, lab)
                del lab
            print('npy: %s (%.2f GB) and %s (%.2f GB), %d segments'
                  % (ip, os.path.getsize(ip) / 1e9, sp, os.path.getsize(sp) / 1e9, S), flush=True)
            hist = np.full(S + 1, BH * BW, dtype=np.int64)
            hist[0] = 0
            measure(source, n, ip, sp, hist)


if __name__ == '__main__':
    main()
