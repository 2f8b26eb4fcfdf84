"""Rank program of tests/test_dist_output_cpu.py (socket transport, no GPU).

  dist_worker_output.py OUTDIR stage JOBS.json
      runDistributed with the oracle engine (tests/dist_output_helpers.py), then writeOutputDistributed; each job
      is {"img", "centres", "msd", "tile", "ov", "minseg", "null", "four", "ranges" (or null), "env", "levels",
      "out"}; rank r writes OUTDIR/<out>_rank<r>.json (its result fields and band statistics)
  dist_worker_output.py OUTDIR errors JOBS.json
      doTiledShepherdSegmentationDistributed with arguments that must fail: each job is {"infile", "outfile",
      "kw", "rankKw" (keywords of one rank only, or null), "out"}; rank r records the exception's type and message
      in OUTDIR/<out>_rank<r>.json and checks that the communicator it passed in is still open"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def stage(comm, outdir, job):
    from oracle import oracle
    from pyshepseg_amd import distributed, shepseg, tiling
    from dist_output_helpers import OutputOracleEngine
    from dist_worker import useRanges
    os.environ.update(job['env'])
    useRanges(distributed, [tuple(r) for r in job['ranges']] if job['ranges'] else None)
    tiling.overviewLevels = lambda xs, ys, lv=list(job['levels']): list(lv)
    img = np.load(job['img'])
    eng = OutputOracleEngine(img, oracle)
    null = job['null']
    r = distributed.runDistributed(eng, comm, img.shape[1], img.shape[2], job['tile'], job['ov'],
                                   minSegmentSize=job['minseg'], maxSpectralDiff=job['msd'], imgNullVal=null,
                                   fourConnected=job['four'], kmeansObj=shepseg.KMeansModel(np.load(job['centres'])))
    stats = distributed.writeOutputDistributed(eng, comm, r, os.path.join(outdir, job['out'] + '.npy'))
    with open(os.path.join(outdir, '%s_rank%d.json' % (job['out'], comm.rank)), 'w') as f:
        json.dump({'maxSegId': r.maxSegId, 'stats': stats, 'tiles': list(r.tileRange), 'outRows': list(r.outRows),
                   'mode': r.stitchMode}, f)


def errors(comm, outdir, job):
    from pyshepseg_amd import distributed
    kw = dict(job['kw'])
    if job.get('rankKw') and str(comm.rank) in job['rankKw']:
        kw.update(job['rankKw'][str(comm.rank)])
    got = None
    try:
        distributed.doTiledShepherdSegmentationDistributed(job['infile'], job['outfile'], comm=comm, **kw)
    except Exception as e:      # noqa: B902  (recorded for the test)
        got = [type(e).__name__, str(e)]
    comm.barrier()              # (the communicator passed in is still open)
    with open(os.path.join(outdir, '%s_rank%d.json' % (job['out'], comm.rank)), 'w') as f:
        json.dump(got, f)


def main():
    from pyshepseg_amd import comm as shpcomm
    (outdir, what, jobsPath) = sys.argv[1:4]
    with open(jobsPath) as f:
        jobs = json.load(f)
    comm = shpcomm.SocketComm()
    for job in jobs:
        (stage if what == 'stage' else errors)(comm, outdir, job)
    comm.close()


if __name__ == '__main__':
    main()
