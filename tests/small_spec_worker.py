"""Child process of tests/test_gpu_small_spec.py: a 4-connected and an 8-connected tiled run of one six-band raster
at once, one Python thread each, so that pass loops of both connectivities are pending together on the walker
stream.  Writes both results, the walker batcher's counters and the pass-loop launches per instance
(shp_small_loop_instances).
Usage: small_spec_worker.py OUT.npz WORKERS"""
import ctypes
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import walk_batch_worker as wbw  # noqa: E402


def image6():
    """(img, centres): the 'uneven' raster of walk_batch_worker.py with its three bands twice, the second copy
    shifted by 1000: six bands, the same partition"""
    img, centres = wbw.image_uneven()
    img6 = np.concatenate([img, (img.astype(np.int64) + 1000).clip(1, 65535).astype(np.uint16)])
    return np.ascontiguousarray(img6), np.concatenate([centres, centres + 1000.0], axis=1)


def main():
    out, workers = sys.argv[1], int(sys.argv[2])
    from pyshepseg_amd import tiling, shepseg, _lib
    img, centres = image6()
    L = _lib.lib()
    stats = np.zeros(6, dtype=np.uint64)
    inst = np.zeros(5, dtype=np.uint64)
    cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=workers)
    ras = tiling.DeviceRaster.fromArray(img)
    res, errs = {}, []

    def run(conn):
        try:
            res[conn] = tiling.doTiledShepherdSegmentation(
                ras, None, tileSize=wbw.TILE, overlapSize=wbw.OVERLAP, minSegmentSize=wbw.MINSEG,
                maxSpectralDiff=wbw.MSD, kmeansObj=shepseg.KMeansModel(centres), fourConnected=conn,
                concurrencyCfg=cfg)
        except BaseException as e:      # (reported by the main thread)
            errs.append(e)

    try:
        assert L.shp_walk_batch_stats(stats.ctypes.data_as(ctypes.c_void_p), 1) == 0
        assert L.shp_small_loop_instances(inst.ctypes.data_as(ctypes.c_void_p), 1) == 0
        threads = [threading.Thread(target=run, args=(conn,)) for conn in (True, False)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errs:
            raise errs[0]
        assert L.shp_walk_batch_stats(stats.ctypes.data_as(ctypes.c_void_p), 0) == 0
        assert L.shp_small_loop_instances(inst.ctypes.data_as(ctypes.c_void_p), 0) == 0
    finally:
        ras.free()
    (a, b) = (res[True], res[False])
    np.savez(out, seg4=a.segimg, hist4=a.hist, max_seg_id4=np.int64(a.maxSegId), seg8=b.segimg, hist8=b.hist,
             max_seg_id8=np.int64(b.maxSegId), stats=stats, inst=inst)


if __name__ == '__main__':
    main()
