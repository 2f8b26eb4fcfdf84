"""Rank program of tests/test_gpu_shapes_dist.py: shape attributes on the multi-rank pipeline, on the synthetic 6-band
1500 x 1300 raster with the HIP engine -- runDistributed (output kept on the device), writeOutputDistributed (the label
file the shapes are compared with), calcSegmentShapesDistributed of the kept output, findSegmentNeighboursDistributed,
mergeSegmentsDistributed by the key column id % 3 with the recoded rows written to a file, and
calcSegmentShapesDistributed of the merge's objects.  Transport 'socket': every rank uses GPU 0; 'rccl': one GPU per
rank.  SHEPSEG_SHARD comes from the environment.  At world size 1 the one-GPU calcSegmentShapes also runs on the same
resident labels, and the device times of both (second runs) are saved.

  dist_worker_shapes_gpu.py OUTDIR TRANSPORT TAG   writes OUTDIR/TAG_labels.npy, TAG_merged.npy and TAG_rank<r>.npz"""
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
    from pyshepseg_amd import distributed, shapes, tiling
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
    s1 = distributed.calcSegmentShapesDistributed(eng, comm, r, info=info)
    (distMs, oneMs) = (s1.deviceMs, -1.0)
    if comm.world == 1:
        # the same kernel on the same resident labels, both a second time (buffers sized, code loaded)
        s1 = distributed.calcSegmentShapesDistributed(eng, comm, r, info=info)
        distMs = s1.deviceMs
        kept = types.SimpleNamespace(outDev=(distributed._addr(eng._lastOut), nr, nc, 0))
        for _ in range(2):
            oneMs = shapes.calcSegmentShapes(kept, maxSegId=r.maxSegId).deviceMs
    share = distributed.findSegmentNeighboursDistributed(eng, comm, r)
    nbCols = share.columns
    keys = np.arange(r.maxSegId + 1, dtype=np.int64) % 3
    m = distributed.mergeSegmentsDistributed(eng, comm, share, keys, dres=r, outfile=base + '_merged.npy')
    info2 = {}
    s2 = distributed.calcSegmentShapesDistributed(eng, comm, m, info=info2)
    tiling.freeDeviceOutput(m)
    eng.releaseOutput()
    out = {'s1_' + k: v for (k, v) in list(s1.columns.items()) + list(s1.sums.items())}
    out.update({'s2_' + k: v for (k, v) in list(s2.columns.items()) + list(s2.sums.items())})
    out.update({'i1_' + k: v for (k, v) in info.items()})
    out.update({'i2_' + k: v for (k, v) in info2.items()})
    np.savez(base + '_rank%d.npz' % comm.rank, outLo=r.outRows[0], outHi=r.outRows[1], maxSegId=r.maxSegId,
             hist=np.asarray(r.hist).astype(np.int64), M=m.maxSegId, newHist=m.hist, deviceMs=distMs, oneGpuMs=oneMs,
             borderLength=nbCols['borderLength'], **out)
    comm.close()


if __name__ == '__main__':
    main()
