"""Rank program of tests/test_gpu_spatial_userfunc_distributed.py: the multi-GPU driver with the HIP engine (ranks
share GPU 0 over the socket transport), then user-defined spatial statistics of its sharded output rows.

  dist_worker_spatial_userfunc_gpu.py OUTDIR NROWS NCOLS TILE OVERLAP BAND NULL
      the synthetic 4-band raster of seed 11; statsR.npz per rank: the columns of every tile size of TILES"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

TILES = [100, 1024]            # visit-order tiles: 100 does not divide the shard boundary (a multiple of 256)
PARAM = 4


def _types():
    from pyshepseg_amd import tilingstats as ts
    return [ts.GFT_Integer, ts.GFT_Real, ts.GFT_Integer]


def main():
    (outdir, nr, nc, tile, ov, bandnum, null) = sys.argv[1:8]
    (nr, nc, tile, ov, bandnum, null) = (int(nr), int(nc), int(tile), int(ov), int(bandnum), int(null))
    os.environ['SHEPSEG_DEVICE'] = '0'
    from pyshepseg_amd import comm as shpcomm, distributed, tiling, tilingstats as ts
    import spatial_userfunc_dist_helpers as U
    comm = shpcomm.SocketComm()

    def makeSlice(yLo, yHi):
        return tiling.DeviceRaster.synth(11, 4, yHi - yLo, nc, y0=yLo, x0=0)
    eng = distributed.HipEngine(makeSlice, numWorkers=2, keepOutput=True)
    r = distributed.runDistributed(eng, comm, nr, nc, tile, ov, minSegmentSize=30, numClusters=20,
                                   fixedKMeansInit=True)
    out = {}
    fn = ts.spatialUserFunc(U.order_hash)
    for t in TILES:
        info = {}
        ic, fc = distributed.calcPerSegmentSpatialStatsDistributed(eng, comm, r.hist, bandnum, _types(), fn, PARAM,
                                                                   imgNullVal=null, info=info, tileSize=t,
                                                                   batchPoints=5000)
        assert info['path'] == 'points'
        out['ic%d' % t], out['fc%d' % t] = ic, fc
        out['straddlers%d' % t] = info['straddlers']
        out['calls%d' % t] = info['calls']
    eng.releaseOutput()
    if eng.ras is not None:
        eng.ras.free()
    np.savez(os.path.join(outdir, 'stats%d.npz' % comm.rank), outLo=r.outRows[0], outHi=r.outRows[1],
             maxSegId=r.maxSegId, mode=r.stitchMode, **out)
    comm.close()


if __name__ == '__main__':
    main()
