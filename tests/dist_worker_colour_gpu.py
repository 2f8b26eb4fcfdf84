"""Rank program of tests/test_gpu_colour_table_dist.py: the multi-rank pipeline from the raster to the picture on
the synthetic 6-band 1500 x 1300 raster with the HIP engine -- runDistributed (output kept on the device),
writeOutputDistributed (the label files the picture is compared with), calcPerSegmentStatsDistributedBands for the
means of bands 1, 3 and 6, statsColumnsByName, writeColorTableFromRatColumnsDistributed,
renderColourTableDistributed(outfile=...).  Transport 'socket': every rank uses GPU 0; 'rccl': one GPU per rank.
SHEPSEG_SHARD / SHEPSEG_STITCH come from the environment; RANGES ('0:3,3:6': one tile range per rank) replaces the
driver's own sharding, e.g. to cut in the middle of a tile row so that two ranks share output rows.

  dist_worker_colour_gpu.py OUTDIR TRANSPORT TAG [RANGES]   writes OUTDIR/TAG_labels.npy, TAG_rgba.npy (and their
                                                            _ov layers) and OUTDIR/TAG_rank<r>.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

BANDS = [1, 3, 6]
LEVELS = [2, 4, 8, 16]
NAMES = ['mean1', 'mean3', 'mean6']


def main():
    (outdir, transport, tag) = sys.argv[1:4]
    os.environ['SHEPSEG_DEVICE'] = '0' if transport == 'socket' else os.environ.get('LOCAL_RANK', '0')
    from pyshepseg_amd import distributed, tiling
    from pyshepseg_amd import comm as shpcomm
    if len(sys.argv) > 4:
        import dist_cases
        from dist_worker import useRanges
        useRanges(distributed, dist_cases.decodeRanges(sys.argv[4]))
    tiling.overviewLevels = lambda xs, ys: list(LEVELS)
    comm = shpcomm.SocketComm() if transport == 'socket' else shpcomm.RcclComm()
    (nb, nr, nc) = (6, 1500, 1300)

    def makeSlice(yLo, yHi):
        return tiling.DeviceRaster.synth(11, nb, yHi - yLo, nc, y0=yLo, x0=0)
    eng = distributed.HipEngine(makeSlice, numWorkers=3, keepOutput=True)
    r = distributed.runDistributed(eng, comm, nr, nc, 512, 128, minSegmentSize=50, numClusters=30, fixedKMeansInit=True)
    base = os.path.join(outdir, tag)
    distributed.writeOutputDistributed(eng, comm, r, base + '_labels.npy')
    entries = [(b, [(name, 'mean'), ('n%d' % b, 'pixcount')]) for (b, name) in zip(BANDS, NAMES)]
    (ic, fc, fast) = distributed.calcPerSegmentStatsDistributedBands(eng, comm, r.hist, entries)
    columns = distributed.statsColumnsByName(entries, ic, fc, fast)
    info = {}
    table = distributed.writeColorTableFromRatColumnsDistributed(eng, comm, columns, *NAMES, info=info)
    onEngine = eng.colourTable is not None and eng.colourTable[1] == r.maxSegId + 1
    rinfo = {}
    # (blocks of about 60 rows: every rank's rows make several blocks and more than one group of them)
    got = distributed.renderColourTableDistributed(eng, comm, r, outfile=base + '_rgba.npy', blockPixels=60 * nc,
                                                   info=rinfo)
    eng.releaseOutput()
    np.savez(base + '_rank%d.npz' % comm.rank, outLo=r.outRows[0], outHi=r.outRows[1], maxSegId=r.maxSegId,
             stretch=np.array(table.stretch, dtype=np.float64), deviceMs=table.deviceMs, onEngine=int(onEngine),
             freed=int(eng.colourTable is None), returned=int(got is None), rows=np.array(info['rows']),
             exchange_bytes=info['exchange_bytes'], blocks=rinfo['blocks'], tiles=np.array(r.tileRange),
             **{k: table.columns[k] for k in table.columns}, **{k: np.asarray(columns[k]) for k in NAMES})
    comm.close()


if __name__ == '__main__':
    main()
