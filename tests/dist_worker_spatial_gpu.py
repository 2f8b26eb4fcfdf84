"""Rank program of tests/test_gpu_spatial_distributed.py: the multi-GPU driver with the HIP engine (ranks share
GPU 0 over the socket transport), then the spatial statistics of its sharded output rows.

  dist_worker_spatial_gpu.py OUTDIR NROWS NCOLS TILE OVERLAP BAND NULL
      the synthetic 4-band raster of seed 11; statsR.npz per rank: every spatial function's columns"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

# (name, function, parameter, column types): the cases the test compares, in this order on every rank
CASES = [('mean', 'userFuncMeanCoord', [300000.0, 10.0, 0.0, 7000000.0, 0.0, -10.0], 'RR'),
         ('meanrot', 'userFuncMeanCoord', [300000.5, 10.25, 0.75, 7000000.25, -0.5, -10.125], 'RR'),
         ('edge4', 'userFuncNumEdgePixels', True, 'I'),
         ('edge8', 'userFuncNumEdgePixels', False, 'I'),
         ('vario5', 'userFuncVariogram', 5, 'RRRRR')]


def main():
    (outdir, nr, nc, tile, ov, bandnum, null) = sys.argv[1:8]
    (nr, nc, tile, ov, bandnum, null) = (int(nr), int(nc), int(tile), int(ov), int(bandnum), int(null))
    os.environ['SHEPSEG_DEVICE'] = '0'
    from pyshepseg_amd import comm as shpcomm, distributed, tiling, tilingstats as ts
    comm = shpcomm.SocketComm()

    def makeSlice(yLo, yHi):
        return tiling.DeviceRaster.synth(11, 4, yHi - yLo, nc, y0=yLo, x0=0)
    eng = distributed.HipEngine(makeSlice, numWorkers=2, keepOutput=True)
    r = distributed.runDistributed(eng, comm, nr, nc, tile, ov, minSegmentSize=30, numClusters=20,
                                   fixedKMeansInit=True)
    out = {}
    for (name, fn, prm, cols) in CASES:
        types = [ts.GFT_Real if t == 'R' else ts.GFT_Integer for t in cols]
        info = {}
        ic, fc = distributed.calcPerSegmentSpatialStatsDistributed(eng, comm, r.hist, bandnum, types,
                                                                   getattr(ts, fn), prm, imgNullVal=null, info=info)
        out[name + '_ic'], out[name + '_fc'] = ic, fc
        out[name + '_straddlers'] = info['straddlers']
        out[name + '_halo'] = info['halo_rows']
    eng.releaseOutput()
    if eng.ras is not None:
        eng.ras.free()
    np.savez(os.path.join(outdir, 'stats%d.npz' % comm.rank), outLo=r.outRows[0], outHi=r.outRows[1],
             maxSegId=r.maxSegId, mode=r.stitchMode, **out)
    comm.close()


if __name__ == '__main__':
    main()
