"""Rank program of tests/test_gpu_distributed.py: the multi-GPU driver with the HIP engine.
Transport 'socket': every rank uses GPU 0 (one-GPU test box), strips staged through host memory;
'rccl': one GPU per rank, strips device to device.

  dist_worker_gpu.py OUTDIR TRANSPORT
      the synthetic 6-band 1500 x 1300 raster, the k-means fit and the statistics of the driver
  dist_worker_gpu.py OUTDIR TRANSPORT npy IMAGE.npy CENTRES.npy MSD TILE OVERLAP MINSEG NULL FOUR [--ranges=...]
      the stitch of an image of the test (NULL -1: none) with the given model; --ranges as in dist_worker.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def runNpy(comm, outdir, args):
    from pyshepseg_amd import distributed, shepseg, tiling
    (imgPath, centresPath, msd, tile, ov, minseg, null, four) = args
    img = np.load(imgPath)
    centres = np.load(centresPath)
    null = None if int(null) < 0 else int(null)

    def makeSlice(yLo, yHi):
        return tiling.DeviceRaster.fromArray(np.ascontiguousarray(img[:, yLo:yHi]), null)
    eng = distributed.HipEngine(makeSlice, numWorkers=2, keepOutput=True)
    r = distributed.runDistributed(eng, comm, img.shape[1], img.shape[2], int(tile), int(ov),
                                   minSegmentSize=int(minseg), maxSpectralDiff=float(msd), imgNullVal=null,
                                   fourConnected=bool(int(four)), kmeansObj=shepseg.KMeansModel(centres))
    out = eng.localOutput()
    eng.releaseOutput()
    if eng.ras is not None:
        eng.ras.free()
    np.savez(os.path.join(outdir, 'rank%d.npz' % comm.rank), out=out, outLo=r.outRows[0], outHi=r.outRows[1],
             maxSegId=r.maxSegId, hist=r.hist, mode=r.stitchMode, redone=r.chainStepsRedone,
             tiles=np.array(r.tileRange))


def main():
    from dist_worker import popRanges, useRanges
    ranges = popRanges(sys.argv)
    outdir, transport = sys.argv[1], sys.argv[2]
    if transport == 'socket':
        os.environ['SHEPSEG_DEVICE'] = '0'
    else:
        os.environ['SHEPSEG_DEVICE'] = os.environ.get('LOCAL_RANK', '0')
    from pyshepseg_amd import distributed, tiling
    useRanges(distributed, ranges)
    from pyshepseg_amd import comm as shpcomm
    comm = shpcomm.SocketComm() if transport == 'socket' else shpcomm.RcclComm()
    if len(sys.argv) > 3 and sys.argv[3] == 'npy':
        runNpy(comm, outdir, sys.argv[4:])
        comm.close()
        return
    nb, nr, nc = 6, 1500, 1300

    def makeSlice(yLo, yHi):
        return tiling.DeviceRaster.synth(11, nb, yHi - yLo, nc, y0=yLo, x0=0)
    eng = distributed.HipEngine(makeSlice, numWorkers=3, keepOutput=True)
    r = distributed.runDistributed(eng, comm, nr, nc, 512, 128, minSegmentSize=50, numClusters=30,
                                   fixedKMeansInit=True)
    out = eng.localOutput()
    sel = [('a', 'min'), ('b', 'max'), ('c', 'mean'), ('d', 'stddev'), ('e', 'median'),
           ('f', 'mode'), ('g', 'percentile', 90), ('h', 'pixcount')]
    ic, fc, _fast = distributed.calcPerSegmentStatsDistributed(eng, comm, r.hist, 3, sel)
    np.savez(os.path.join(outdir, 'stats%d.npz' % comm.rank), ic=ic, fc=fc)
    eng.releaseOutput()
    np.savez(os.path.join(outdir, 'rank%d.npz' % comm.rank), out=out, outLo=r.outRows[0],
             outHi=r.outRows[1], maxSegId=r.maxSegId, hist=r.hist,
             centres=r.kmeans.cluster_centers_, msd=r.maxSpectralDiff, mode=r.stitchMode)
    comm.close()


if __name__ == '__main__':
    main()
