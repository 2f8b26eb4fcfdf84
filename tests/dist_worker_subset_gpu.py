"""Rank program of tests/test_gpu_subset_distributed.py: the multi-GPU driver with the HIP engine (ranks share GPU 0
over the socket transport), then subsetImageDistributed of its sharded output rows with a mask and a .npy output.

  dist_worker_subset_gpu.py OUTDIR NROWS NCOLS TILE OVERLAP
      the synthetic 4-band raster of seed 11; OUTDIR/mask.npy: the window's mask; writes OUTDIR/sub.npy (all
      ranks) and subsetR.npz per rank"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

WINDOW = (37, 100, 500, 550)       # (tlx, tly, xs, ys): crosses the rank boundary (a multiple of 256)


def column(maxSegId):
    return np.arange(maxSegId + 1, dtype=np.float64) * 0.5 + 7


def main():
    (outdir, nr, nc, tile, ov) = sys.argv[1:6]
    (nr, nc, tile, ov) = (int(nr), int(nc), int(tile), int(ov))
    os.environ['SHEPSEG_DEVICE'] = '0'
    from pyshepseg_amd import comm as shpcomm, distributed, tiling
    comm = shpcomm.SocketComm()

    def makeSlice(yLo, yHi):
        return tiling.DeviceRaster.synth(11, 4, yHi - yLo, nc, y0=yLo, x0=0)
    eng = distributed.HipEngine(makeSlice, numWorkers=2, keepOutput=True)
    r = distributed.runDistributed(eng, comm, nr, nc, tile, ov, minSegmentSize=30, numClusters=20,
                                   fixedKMeansInit=True)
    (tlx, tly, xs, ys) = WINDOW
    res = distributed.subsetImageDistributed(eng, comm, r, tlx, tly, xs, ys, outname=os.path.join(outdir, 'sub.npy'),
                                             origSegIdColName='orig', maskImage=os.path.join(outdir, 'mask.npy'),
                                             ratColumns={'v': column(r.maxSegId)})
    eng.releaseOutput()
    if eng.ras is not None:
        eng.ras.free()
    cols = {'col_' + k: v for (k, v) in res.columns.items()}
    np.savez(os.path.join(outdir, 'subset%d.npz' % comm.rank), outLo=r.outRows[0], outHi=r.outRows[1],
             maxSegId=r.maxSegId, rows=res.segimg, a=res.rows[0], b=res.rows[1], orig=res.origSegIds, hist=res.hist,
             **cols)
    comm.close()


if __name__ == '__main__':
    main()
