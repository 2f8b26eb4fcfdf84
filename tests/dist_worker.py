"""Rank program of tests/test_distributed_cpu.py (socket transport, no GPU): runs the multi-GPU driver with
the oracle engine and writes this rank's output rows to disk.

  dist_worker.py OUTDIR TILE OVERLAP SIMPLE [FIXTURE] [--ranges=T0:T1,T0:T1,...]
  dist_worker.py OUTDIR cases JOBS.json

--ranges: the ranks' [t0, t1) tile ranges instead of what distributed.shardTiles picks (one per rank).
`cases`: a list of stitch runs over one communicator, each {"fixture", "ranges" (or null), "env", "out"};
rank r writes OUTDIR/<out>_rank<r>.npz."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

_shardTiles = None          # distributed.shardTiles itself


def popRanges(argv):
    """the ranges of a --ranges=T0:T1,... argument (removed from argv), or None"""
    ranges = None
    for a in list(argv):
        if a.startswith('--ranges='):
            ranges = [tuple(int(v) for v in p.split(':')) for p in a[len('--ranges='):].split(',')]
            argv.remove(a)
    return ranges


def useRanges(distributed, ranges):
    """Make the driver shard by `ranges` (None: by shardTiles itself).  runDistributed looks shardTiles up in
    the module's globals, so replacing the module attribute is enough."""
    global _shardTiles
    if _shardTiles is None:
        _shardTiles = distributed.shardTiles
    if ranges is None:
        distributed.shardTiles = _shardTiles
        return

    def fixed(tileInfo, world, wholeRows=False):
        assert len(ranges) == world and ranges[-1][1] == tileInfo.ncols * tileInfo.nrows, (ranges, world)
        return [tuple(r) for r in ranges]
    distributed.shardTiles = fixed


def runFixture(comm, path, outfile):
    """a stitch fixture: the image, model and parameters of an .npz; only the stitch's results are written"""
    from oracle import oracle
    from pyshepseg_amd import distributed, shepseg
    from dist_oracle_engine import OracleEngine
    g = np.load(path, allow_pickle=True)
    img = g['img']
    eng = OracleEngine(img, oracle)
    r = distributed.runDistributed(
        eng, comm, img.shape[1], img.shape[2], int(g['tile_size']), int(g['overlap']),
        minSegmentSize=int(g['min_seg']), maxSpectralDiff=float(g['msd']),
        imgNullVal=(int(g['null_val']) if int(g['has_null']) else None),
        fourConnected=bool(int(g['four'])), kmeansObj=shepseg.KMeansModel(g['centres']))
    np.savez(outfile, out=eng.out, outLo=r.outRows[0], outHi=r.outRows[1], maxSegId=r.maxSegId, hist=r.hist,
             mode=r.stitchMode, redone=r.chainStepsRedone, ntiles=r.numTileRows * r.numTileCols,
             tiles=np.array(r.tileRange))


def main():
    from pyshepseg_amd import distributed
    useRanges(distributed, popRanges(sys.argv))
    outdir = sys.argv[1]
    if sys.argv[2] == 'cases':
        import json
        from pyshepseg_amd import comm as shpcomm
        comm = shpcomm.SocketComm()
        with open(sys.argv[3]) as f:
            jobs = json.load(f)
        for job in jobs:
            os.environ.update(job['env'])
            useRanges(distributed, job['ranges'])
            runFixture(comm, job['fixture'], os.path.join(outdir, '%s_rank%d.npz' % (job['out'], comm.rank)))
        comm.close()
        return

    tile, ov, simple = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    from oracle import oracle
    from pyshepseg_amd import comm as shpcomm
    from dist_oracle_engine import OracleEngine
    comm = shpcomm.SocketComm()
    golden = sys.argv[5] if len(sys.argv) > 5 else None
    if golden:
        runFixture(comm, golden, os.path.join(outdir, 'rank%d.npz' % comm.rank))
        comm.close()
        return
    img = np.load(os.path.join(outdir, 'img.npy'))
    eng = OracleEngine(img, oracle)
    r = distributed.runDistributed(eng, comm, img.shape[1], img.shape[2], tile, ov,
                                   minSegmentSize=12, numClusters=8, fixedKMeansInit=True,
                                   simpleTileRecode=bool(simple))
    sel = [('a', 'min'), ('b', 'max'), ('c', 'mean'), ('d', 'stddev'), ('e', 'median'),
           ('f', 'mode'), ('g', 'percentile', 25), ('h', 'pixcount')]
    info = {}
    ic, fc, _fast = distributed.calcPerSegmentStatsDistributed(eng, comm, r.hist, 2, sel,
                                                               imgNullVal=65535, info=info)
    np.savez(os.path.join(outdir, 'stats%d.npz' % comm.rank), ic=ic, fc=fc, straddlers=info['straddlers'],
             straddler_pixels=info['straddler_pixels'])
    np.savez(os.path.join(outdir, 'rank%d.npz' % comm.rank), out=eng.out, outLo=r.outRows[0],
             outHi=r.outRows[1], maxSegId=r.maxSegId, hist=r.hist,
             centres=r.kmeans.cluster_centers_, msd=r.maxSpectralDiff, rows=np.array(r.rowRange),
             mode=r.stitchMode)
    comm.close()


if __name__ == '__main__':
    main()
