"""Child process of tests/test_gpu_walk_batch.py: segments the test's raster with the tiled driver under the
knobs of its own environment and writes labels, histogram, maxSegId and the walker batcher's counters.
Usage: walk_batch_worker.py OUT.npz FOUR WORKERS"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import seg_cases  # noqa: E402

NR, NC = 1024, 1280
BASE = np.array([[0, 0, 0], [9000, 12000, 15000], [14000, 9000, 20000], [20000, 22000, 8000],
                 [26000, 15000, 12000], [30000, 30000, 30000]], dtype=np.int64)
TILE, OVERLAP, MINSEG, MSD = 256, 64, 30, 1e9


def image():
    """(img, centres): cut_components' cluster codes with a 16 x 16 chequerboard in the first tile's core (so that
    tile holds no component above the depth-first cut's cap when 4-connected), as spectra with 3 % outliers and
    +-40 noise"""
    cl = seg_cases.cut_components(NR, NC)
    yy, xx = np.mgrid[0:256, 0:256]
    cl[:256, :256] = 1 + ((yy // 16 + xx // 16) % 2)
    rng = np.random.RandomState(33)
    flip = rng.rand(NR, NC) < 0.03
    cl[flip] = rng.randint(1, 6, size=int(flip.sum()))
    img = BASE[cl].transpose(2, 0, 1) + rng.randint(-40, 41, size=(3, NR, NC))
    return np.ascontiguousarray(np.clip(img, 1, 65535).astype(np.uint16)), BASE[1:].astype(np.float64)


def main():
    out, four, workers = sys.argv[1], bool(int(sys.argv[2])), int(sys.argv[3])
    from pyshepseg_amd import tiling, shepseg, _lib
    img, centres = image()
    L = _lib.lib()
    stats = np.zeros(6, dtype=np.uint64)
    cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=workers)
    ras = tiling.DeviceRaster.fromArray(img)
    try:
        assert L.shp_walk_batch_stats(stats.ctypes.data_as(ctypes.c_void_p), 1) == 0
        r = tiling.doTiledShepherdSegmentation(ras, None, tileSize=TILE, overlapSize=OVERLAP, minSegmentSize=MINSEG,
                                               maxSpectralDiff=MSD, kmeansObj=shepseg.KMeansModel(centres),
                                               fourConnected=four, concurrencyCfg=cfg)
        assert L.shp_walk_batch_stats(stats.ctypes.data_as(ctypes.c_void_p), 0) == 0
    finally:
        ras.free()
    np.savez(out, seg=r.segimg, hist=r.hist, max_seg_id=np.int64(r.maxSegId), stats=stats)


if __name__ == '__main__':
    main()
