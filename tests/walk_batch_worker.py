"""Child process of tests/test_gpu_walk_batch.py and tests/test_gpu_walk_batch_uneven.py: segments one of the
tests' rasters with the tiled driver under the knobs of its own environment and writes labels, histogram,
maxSegId, the walker batcher's counters (launches, jobs, largest batch; workgroup sum, most workgroups in a launch;
per class) and the replay's and the pass loop's profile sums over the worker contexts.
Usage: walk_batch_worker.py OUT.npz FOUR WORKERS [RASTER]
FOUR = 1 | 0 runs one connectivity; FOUR = both runs a 4-connected and an 8-connected tiled run at once, one Python
thread each, and writes seg4 / hist4 / max_seg_id4 and seg8 / hist8 / max_seg_id8."""
import ctypes
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import seg_cases  # noqa: E402

NR, NC = 1024, 1280
BASE = np.array([[0, 0, 0], [9000, 12000, 15000], [14000, 9000, 20000], [20000, 22000, 8000],
                 [26000, 15000, 12000], [30000, 30000, 30000]], dtype=np.int64)
TILE, OVERLAP, MINSEG, MSD = 256, 64, 30, 1e9
PROF_DFS, PROF_SMALL_LOOP = 2, 5


def _spectra(cl, seed):
    """cluster codes as spectra with 3 % outliers and +-40 noise"""
    rng = np.random.RandomState(seed)
    flip = rng.rand(NR, NC) < 0.03
    cl[flip] = rng.randint(1, 6, size=int(flip.sum()))
    img = BASE[cl].transpose(2, 0, 1) + rng.randint(-40, 41, size=(3, NR, NC))
    return np.ascontiguousarray(np.clip(img, 1, 65535).astype(np.uint16)), BASE[1:].astype(np.float64)


def image():
    """(img, centres): cut_components' cluster codes with a 16 x 16 chequerboard in the first tile's core (so that
    tile holds no component above the depth-first cut's cap when 4-connected), as spectra with 3 % outliers and
    +-40 noise"""
    cl = seg_cases.cut_components(NR, NC)
    yy, xx = np.mgrid[0:256, 0:256]
    cl[:256, :256] = 1 + ((yy // 16 + xx // 16) % 2)
    return _spectra(cl, 33)


def image_uneven():
    """(img, centres): tiles that differ widely in their number of components above the depth-first cut's cap
    (tests/walk_batch_cases.py counts them).  Vertical stripes 26 pixels wide left of column 640 -- too narrow to
    reach the cap in a tile of the upper rows, wide enough in the taller tiles of the last tile row -- and 52 wide
    from there; the other raster's chequerboard in the first tile's core; a four-row bar across everything that
    cuts the stripes of the tiles it crosses."""
    cl = np.empty((NR, NC), dtype=np.int32)
    x = np.arange(NC)
    cl[:] = np.where(x < 640, 1 + (x // 26) % 2, 3 + (x // 52) % 2)[None, :]
    yy, xx = np.mgrid[0:256, 0:256]
    cl[:256, :256] = 1 + ((yy // 16 + xx // 16) % 2)
    cl[600:604, :] = 5
    return _spectra(cl, 34)


IMAGES = {'even': image, 'uneven': image_uneven}


def main():
    out, four, workers = sys.argv[1], sys.argv[2], int(sys.argv[3])
    raster = sys.argv[4] if len(sys.argv) > 4 else 'even'
    from pyshepseg_amd import tiling, shepseg, _lib
    img, centres = IMAGES[raster]()
    L = _lib.lib()
    stats = np.zeros(6, dtype=np.uint64)
    blocks = np.zeros(4, dtype=np.uint64)
    cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=workers)
    ras = tiling.DeviceRaster.fromArray(img)
    res, errs = {}, []

    def run(conn):
        try:
            res[conn] = tiling.doTiledShepherdSegmentation(
                ras, None, tileSize=TILE, overlapSize=OVERLAP, minSegmentSize=MINSEG, maxSpectralDiff=MSD,
                kmeansObj=shepseg.KMeansModel(centres), fourConnected=conn, concurrencyCfg=cfg)
        except BaseException as e:      # (reported by the main thread)
            errs.append(e)

    try:
        assert L.shp_walk_batch_stats(stats.ctypes.data_as(ctypes.c_void_p), 1) == 0
        if four == 'both':
            threads = [threading.Thread(target=run, args=(conn,)) for conn in (True, False)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        else:
            run(bool(int(four)))
        if errs:
            raise errs[0]
        assert L.shp_walk_batch_stats(stats.ctypes.data_as(ctypes.c_void_p), 0) == 0
        assert L.shp_walk_batch_blocks(blocks.ctypes.data_as(ctypes.c_void_p)) == 0
        # the workers' contexts are back in the pool: their profile sums, as bench.py takes them
        prof_ms, prof_cnt = np.zeros(16), np.zeros(16, dtype=np.uint64)
        for c in _lib.pool_contexts():
            ms = (ctypes.c_double * 16)()
            cnt = (ctypes.c_uint64 * 16)()
            c.check(L.shp_prof_get(c.handle, ms, cnt, 16, 0))
            prof_ms += np.array(ms[:])
            prof_cnt += np.array(cnt[:], dtype=np.uint64)
    finally:
        ras.free()
    prof = dict(prof_ms=prof_ms[[PROF_DFS, PROF_SMALL_LOOP]], prof_cnt=prof_cnt[[PROF_DFS, PROF_SMALL_LOOP]])
    if four == 'both':
        (a, b) = (res[True], res[False])
        np.savez(out, seg4=a.segimg, hist4=a.hist, max_seg_id4=np.int64(a.maxSegId), seg8=b.segimg, hist8=b.hist,
                 max_seg_id8=np.int64(b.maxSegId), stats=stats, blocks=blocks, **prof)
    else:
        r = res[bool(int(four))]
        np.savez(out, seg=r.segimg, hist=r.hist, max_seg_id=np.int64(r.maxSegId), stats=stats, blocks=blocks, **prof)


if __name__ == '__main__':
    main()
