"""Rank program of tests/test_gpu_stats_bands_dist.py: the multi-GPU driver with the HIP engine on the synthetic
6-band 1500 x 1300 raster, then calcPerSegmentStatsDistributedBands for bands 1, 3 and 6 and one
calcPerSegmentStatsDistributed call per band from the same run.  Transport 'socket': every rank uses GPU 0 (the host
path, HipEngine's ...Bands methods); 'rccl': one GPU per rank (the device path).

  dist_worker_stats_bands_gpu.py OUTDIR TRANSPORT      writes OUTDIR/bands<rank>.npz and rank<rank>.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

BANDS = [1, 3, 6]


def selectionOf(b):
    return [('mean%d' % b, 'mean'), ('sd%d' % b, 'stddev'), ('med%d' % b, 'median'), ('n%d' % b, 'pixcount')]


def main():
    (outdir, transport) = (sys.argv[1], sys.argv[2])
    os.environ['SHEPSEG_DEVICE'] = '0' if transport == 'socket' else os.environ.get('LOCAL_RANK', '0')
    from pyshepseg_amd import distributed, tiling
    from pyshepseg_amd import comm as shpcomm
    comm = shpcomm.SocketComm() if transport == 'socket' else shpcomm.RcclComm()
    (nb, nr, nc) = (6, 1500, 1300)

    def makeSlice(yLo, yHi):
        return tiling.DeviceRaster.synth(11, nb, yHi - yLo, nc, y0=yLo, x0=0)
    eng = distributed.HipEngine(makeSlice, numWorkers=3, keepOutput=True)
    r = distributed.runDistributed(eng, comm, nr, nc, 512, 128, minSegmentSize=50, numClusters=30, fixedKMeansInit=True)
    out = eng.localOutput()
    info = {}
    (ic, fc, fast) = distributed.calcPerSegmentStatsDistributedBands(eng, comm, r.hist, [(b, selectionOf(b)) for b in BANDS],
                                                                     info=info)
    res = dict(ic=ic, fc=fc, fast=fast, path=info['path'], bands=info['bands'], straddlers=info['straddlers'],
               straddler_pixels=info['straddler_pixels'], exchange_bytes=info['exchange_bytes'])
    for b in BANDS:
        one = {}
        (ic1, fc1, _f) = distributed.calcPerSegmentStatsDistributed(eng, comm, r.hist, b, selectionOf(b), info=one)
        res.update({'ic%d' % b: ic1, 'fc%d' % b: fc1, 'path%d' % b: one['path'], 'straddlers%d' % b: one['straddlers'],
                    'straddler_pixels%d' % b: one['straddler_pixels']})
    eng.releaseOutput()
    np.savez(os.path.join(outdir, 'bands%d.npz' % comm.rank), **res)
    np.savez(os.path.join(outdir, 'rank%d.npz' % comm.rank), out=out, outLo=r.outRows[0], outHi=r.outRows[1],
             maxSegId=r.maxSegId, hist=r.hist)
    comm.close()


if __name__ == '__main__':
    main()
