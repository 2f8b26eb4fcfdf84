"""The raster of tests/test_spectra_batch_census.py and tests/test_gpu_spectra_batch.py, and the child process that
segments it.

The spectra of the segments above 64 pixels (csrc/elim_small.h k_big_seg_list, k_spectra_big) in tiled runs, where
the tiles of one launch of the pass loop behind them differ in what that kernel has to do.  The raster
is one row of four tile windows (512 rows, tile 512, overlap 64) and repeats, every 448 columns, a pattern without
noise in the cluster codes, so that the segments the spectra stage sees are the clumps drawn here:
  columns   0-159   eight stripes of 20 columns over the whole height (10 240 pixels each, which the clump stage's
                    depth-first cut leaves as pieces of ~10 000 pixels and a rest): four with values near
                    65535, where the float32 sum stops being exact (2^24) after ~260 pixels and the ordered phase
                    does most of the work, four with values below 1500, where 10 240 pixels never reach 2^24;
  columns 160-303   a host field of mid values holding blocks of 65 pixels (the smallest segment that goes to this
                    kernel), 512 and 513 pixels (one and two groups of the exact phase) with values near 65535;
  columns 304-447   a host field of values below 1500 holding the same three blocks with values below 1500;
  3 x 3 blobs       across stripe boundaries: below minSegmentSize, so the pass loop merges each into the neighbour
                    with the nearest mean spectrum -- the labels depend on the sums.
As a program: spectra_batch_cases.py OUT.npz MODE WORKERS with MODE = four | eight (uint16, six bands), bands10
(uint16, ten bands: two band groups at SPECTRA_BG 8) or mixed (a uint8 and a uint16 run at once, one thread each)."""
import ctypes
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

NR, NC = 512, 1920
TILE, OVERLAP, MINSEG, MSD = 512, 64, 30, 1e9
PERIOD = 448
BIG = 64                    # csrc/elim_small.h: segments above this many pixels go to k_spectra_big
EXACT_GROUP = 512           # ... whose exact phase checks its bound once per this many pixels
BOUND = 1 << 24
# cluster codes 1-6: high A, high B, low A, low B, mid (host), blob; (base, step per band) per pixel type
LEVELS = {
    'uint16': ((65200, -20), (62500, -20), (1200, 20), (500, 20), (30000, -20), (42000, -20)),
    'uint8': ((250, -1), (236, -1), (22, 1), (8, 1), (120, -1), (165, -1)),
}
NOISE = {'uint16': 10, 'uint8': 1}
# (row, column in the host field, rows, columns, one more pixel below its first column, code in the mid host, in the low host)
BLOCKS = ((20, 10, 5, 13, 0, 1, 4), (40, 10, 16, 32, 0, 2, 4), (70, 10, 16, 32, 1, 1, 4))


def centres_of(dtype, nb):
    return np.array([[base + step * b for b in range(nb)] for (base, step) in LEVELS[dtype]], dtype=np.float64)


def codes():
    """cluster codes 1-6 of the raster"""
    x = np.arange(NC) % PERIOD
    row = np.where(x < 80, 1 + (x // 20) % 2, np.where(x < 160, 3 + (x // 20) % 2, np.where(x < 304, 5, 3)))
    cl = np.repeat(row[None, :], NR, axis=0).astype(np.int32)
    for x0 in range(0, NC, PERIOD):
        for (host, which) in ((160, 5), (304, 6)):
            for blk in BLOCKS:
                (r, c, h, w, extra) = blk[:5]
                c0 = x0 + host + c
                if c0 + w + 1 > NC:
                    continue
                cl[r:r + h, c0:c0 + w] = blk[which]
                if extra:
                    cl[r + h, c0] = blk[which]
        for (k, bx) in enumerate((19, 59, 99, 159, 303)):
            if x0 + bx + 2 <= NC:
                cl[100 + 40 * k:103 + 40 * k, x0 + bx - 1:x0 + bx + 2] = 6
    return cl


def image(dtype='uint16', nb=6):
    """(img (bands, rows, cols), centres)"""
    cen = centres_of(dtype, nb)
    rng = np.random.RandomState(36 + nb)
    img = cen[codes() - 1].transpose(2, 0, 1).astype(np.int64)
    img += rng.randint(-NOISE[dtype], NOISE[dtype] + 1, size=img.shape)
    return np.ascontiguousarray(img.astype(dtype)), cen


def main():
    out, mode, workers = sys.argv[1], sys.argv[2], int(sys.argv[3])
    from pyshepseg_amd import tiling, shepseg, _lib
    L = _lib.lib()
    runs = {'four': [('uint16', 6, True)], 'eight': [('uint16', 6, False)], 'bands10': [('uint16', 10, True)],
            'mixed': [('uint8', 6, True), ('uint16', 6, True)]}[mode]
    cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=workers)
    rasters, res, errs = [], {}, []
    stats = np.zeros(6, dtype=np.uint64)

    def run(i, ras, cen, four):
        try:
            res[i] = tiling.doTiledShepherdSegmentation(
                ras, None, tileSize=TILE, overlapSize=OVERLAP, minSegmentSize=MINSEG, maxSpectralDiff=MSD,
                kmeansObj=shepseg.KMeansModel(cen), fourConnected=four, concurrencyCfg=cfg)
        except BaseException as e:      # (reported by the main thread)
            errs.append(e)

    try:
        threads = []
        for (i, (dtype, nb, four)) in enumerate(runs):
            img, cen = image(dtype, nb)
            rasters.append(tiling.DeviceRaster.fromArray(img))
            threads.append(threading.Thread(target=run, args=(i, rasters[-1], cen, four)))
        assert L.shp_walk_batch_stats(stats.ctypes.data_as(ctypes.c_void_p), 1) == 0
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errs:
            raise errs[0]
        assert L.shp_walk_batch_stats(stats.ctypes.data_as(ctypes.c_void_p), 0) == 0
    finally:
        for ras in rasters:
            ras.free()
    arrays = {'stats': stats}
    for (i, r) in res.items():
        arrays.update({'seg%d' % i: r.segimg, 'hist%d' % i: r.hist, 'max_seg_id%d' % i: np.int64(r.maxSegId)})
    np.savez(out, **arrays)


if __name__ == '__main__':
    main()
