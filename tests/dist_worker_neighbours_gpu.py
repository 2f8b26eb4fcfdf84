"""Rank program of tests/test_gpu_neighbours_dist.py: the multi-rank pipeline from the raster to neighbour context on
the synthetic 6-band 1500 x 1300 raster with the HIP engine -- runDistributed (output kept on the device),
writeOutputDistributed (the label file the table is compared with), findSegmentNeighboursDistributed,
calcPerSegmentStatsDistributedBands for the mean of band 1, reduceOverNeighboursDistributed for its bordermean and
nearest.  Transport 'socket': every rank uses GPU 0; 'rccl': one GPU per rank.  SHEPSEG_SHARD comes from the
environment.  At world size 1 the one-GPU findSegmentNeighbours also runs on the same resident labels, and the
device times of both (second runs) are saved.

  dist_worker_neighbours_gpu.py OUTDIR TRANSPORT TAG   writes OUTDIR/TAG_labels.npy and OUTDIR/TAG_rank<r>.npz"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    (outdir, transport, tag) = sys.argv[1:4]
    os.environ['SHEPSEG_DEVICE'] = '0' if transport == 'socket' else os.environ.get('LOCAL_RANK', '0')
    from pyshepseg_amd import distributed, neighbours, tiling
    from pyshepseg_amd import comm as shpcomm
    tiling.overviewLevels = lambda xs, ys: []
    comm = shpcomm.SocketComm() if transport == 'socket' else shpcomm.RcclComm()
    (nb, nr, nc) = (6, 1500, 1300)

    def makeSlice(yLo, yHi):
        return tiling.DeviceRaster.synth(11, nb, yHi - yLo, nc, y0=yLo, x0=0)
    eng = distributed.HipEngine(makeSlice, numWorkers=3, keepOutput=True)
    r = distributed.runDistributed(eng, comm, nr, nc, 512, 128, minSegmentSize=50, numClusters=30, fixedKMeansInit=True)
    base = os.path.join(outdir, tag)
    distributed.writeOutputDistributed(eng, comm, r, base + '_labels.npy')
    info = {}
    share = distributed.findSegmentNeighboursDistributed(eng, comm, r, info=info)
    (distMs, oneMs) = (share.deviceMs, -1.0)
    if comm.world == 1:
        # the same kernels on the same resident labels, both a second time (buffers sized, code loaded)
        share = distributed.findSegmentNeighboursDistributed(eng, comm, r, info=info)
        distMs = share.deviceMs
        kept = types.SimpleNamespace(outDev=(distributed._addr(eng._lastOut), nr, nc, 0))
        for _ in range(2):
            oneMs = neighbours.findSegmentNeighbours(kept, maxSegId=r.maxSegId).deviceMs
    entries = [(1, [('mean1', 'mean')])]
    (ic, fc, fast) = distributed.calcPerSegmentStatsDistributedBands(eng, comm, r.hist, entries)
    mean1 = np.ascontiguousarray(distributed.statsColumnsByName(entries, ic, fc, fast)['mean1'])
    out = distributed.reduceOverNeighboursDistributed(eng, comm, share, [(mean1, [('bm', 'bordermean'), ('near', 'nearest')])])
    eng.releaseOutput()
    np.savez(base + '_rank%d.npz' % comm.rank, outLo=r.outRows[0], outHi=r.outRows[1], maxSegId=r.maxSegId,
             idLo=share.idRange[0], idHi=share.idRange[1], offsets=share.offsets, neighbours=share.neighbours,
             borderLengths=share.borderLengths, mean1=mean1, deviceMs=distMs, oneGpuMs=oneMs,
             reduceMs=share.reduceTimings['deviceMs'], **share.columns, **out, **info)
    comm.close()


if __name__ == '__main__':
    main()
