"""Rank program of tests/test_gpu_dist_output.py: distributed.doTiledShepherdSegmentationDistributed on the GPU.
Transport 'socket': every rank uses GPU 0 and one SocketComm passed in; 'rccl': an RcclComm passed in; 'env': the
entry point takes comm.fromEnvironment() itself (world size 1: LocalComm).

  dist_worker_output_gpu.py OUTDIR TRANSPORT JOBS.json
      each job: {"infile", "outfile", "kw" (keywords; "centres": a .npy path -> kmeansObj), "env", "levels" (or
      null), "ranges" (or null), "stats" (imgbandnum for calcPerSegmentStatsDistributed with keepOutput=True, or
      null), "out"}; rank r writes OUTDIR/<out>_rank<r>.npz (result fields) or, when the call raised,
      OUTDIR/<out>_rank<r>.err (type and message)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

SEL = [('a', 'min'), ('b', 'max'), ('c', 'mean'), ('d', 'stddev'), ('e', 'median'), ('f', 'mode'),
       ('g', 'percentile', 90), ('h', 'pixcount')]


def runJob(comm, rank, outdir, job):
    from pyshepseg_amd import distributed, shepseg, tiling
    from dist_worker import useRanges
    os.environ.update(job.get('env') or {})
    useRanges(distributed, [tuple(r) for r in job['ranges']] if job.get('ranges') else None)
    if job.get('levels') is not None:
        tiling.overviewLevels = lambda xs, ys, lv=list(job['levels']): list(lv)
    kw = dict(job['kw'])
    if 'centres' in kw:
        kw['kmeansObj'] = shepseg.KMeansModel(np.load(kw.pop('centres')))
    kw['concurrencyCfg'] = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=3)
    keep = job.get('stats') is not None
    try:
        r = distributed.doTiledShepherdSegmentationDistributed(job['infile'], job['outfile'], comm=comm,
                                                               keepOutput=keep, **kw)
    except Exception as e:      # noqa: B902  (recorded for the test)
        with open(os.path.join(outdir, '%s_rank%d.err' % (job['out'], rank)), 'w') as f:
            json.dump([type(e).__name__, str(e)], f)
        return
    extra = {}
    if keep:
        try:
            ic, fc, _fast = distributed.calcPerSegmentStatsDistributed(r.engine, r.engine.comm, r.hist, job['stats'],
                                                                       SEL)
            extra = dict(ic=ic, fc=fc)
        finally:
            r.engine.release()
    np.savez(os.path.join(outdir, '%s_rank%d.npz' % (job['out'], rank)), maxSegId=r.maxSegId, hist=r.hist,
             centres=r.kmeans.cluster_centers_, msd=r.maxSpectralDiff,
             subsamplePcnt=-1.0 if r.subsamplePcnt is None else r.subsamplePcnt, numTileRows=r.numTileRows,
             numTileCols=r.numTileCols, hasEmpty=r.hasEmptySegments,
             stats=np.array(['%s=%s' % kv for kv in r.bandStatistics]), mode=r.stitchMode,
             redone=r.chainStepsRedone, tiles=np.array(r.tileRange), outRows=np.array(r.outRows),
             rows=np.array(r.rowRange), timings=json.dumps(r.timings.makeSummaryDict()),
             noSeg=int(r.segimg is None and r.overviews is None), **extra)


def main():
    (outdir, transport, jobsPath) = sys.argv[1:4]
    os.environ['SHEPSEG_DEVICE'] = '0' if transport != 'rccl' else os.environ.get('LOCAL_RANK', '0')
    from pyshepseg_amd import comm as shpcomm
    with open(jobsPath) as f:
        jobs = json.load(f)
    comm = None
    if transport == 'socket':
        comm = shpcomm.SocketComm()
    elif transport == 'rccl':
        comm = shpcomm.RcclComm()
    rank = comm.rank if comm is not None else int(os.environ.get('RANK', '0'))
    for job in jobs:
        runJob(comm, rank, outdir, job)
    if comm is not None:
        comm.close()


if __name__ == '__main__':
    main()
