"""Rank program of tests/test_stats_bands_dist_cpu.py (socket transport, oracle engine, no GPU): the multi-rank
driver on OUTDIR/img.npy, then calcPerSegmentStatsDistributedBands against one calcPerSegmentStatsDistributed call
per entry in the same process.

  dist_worker_stats_bands.py OUTDIR TILE OVERLAP          writes OUTDIR/bands<rank>.npz and rank<rank>.npz
  dist_worker_stats_bands.py OUTDIR TILE OVERLAP errors   every bad argument, and a stale histogram in the one-band
                                                          call, must raise on this rank; then exits 0"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

# three entries over two distinct bands: band 2 twice with different null values, different selections per entry,
# all eight statistics somewhere
ENTRIES = [(2, [('a_min', 'min'), ('a_mean', 'mean'), ('a_med', 'median'), ('a_n', 'pixcount')]),
           (3, [('b_max', 'max'), ('b_sd', 'stddev'), ('b_mode', 'mode')]),
           (2, [('c_p25', 'percentile', 25), ('c_n', 'pixcount'), ('c_sd', 'stddev'), ('c_min', 'min')])]
NULLS = [65535, None, 1234]

BAD_ARGUMENTS = [
    ('empty list', dict(bandSelections=[])),
    ('duplicate column name', dict(bandSelections=[(1, [('x', 'min')]), (2, [('x', 'max')])])),
    ('band out of range', dict(bandSelections=[(1, [('x', 'min')]), (9, [('y', 'max')])])),
    ('band zero', dict(bandSelections=[(0, [('x', 'min')]), (2, [('y', 'max')])])),
    ('null list of the wrong length', dict(bandSelections=ENTRIES, imgNullVal=[1, 2])),
]
STALE_HISTOGRAM = 'stale histogram, one band'


def main():
    (outdir, tile, ov) = (sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
    from oracle import oracle
    from pyshepseg_amd import comm as shpcomm
    from pyshepseg_amd import distributed, tilingstats
    from dist_oracle_engine import OracleEngine
    comm = shpcomm.SocketComm()
    img = np.load(os.path.join(outdir, 'img.npy'))
    eng = OracleEngine(img, oracle)
    r = distributed.runDistributed(eng, comm, img.shape[1], img.shape[2], tile, ov, minSegmentSize=12, numClusters=8,
                                   fixedKMeansInit=True)
    if len(sys.argv) > 4 and sys.argv[4] == 'errors':
        for (what, kw) in BAD_ARGUMENTS:
            try:
                distributed.calcPerSegmentStatsDistributedBands(eng, comm, r.hist, **kw)
            except tilingstats.PyShepSegStatsError as e:
                sys.stderr.write('rank %d, %s: %s\n' % (comm.rank, what, e))
            else:
                raise AssertionError('%s did not raise' % what)
        # the one-band call with a histogram that gives one id (whole on a rank) a pixel fewer than that rank holds:
        # the rank that holds it finds out, every rank raises
        lh = np.asarray(eng.histogram(r.maxSegId)).astype(np.int64)
        whole = np.flatnonzero((lh[1:] == np.asarray(r.hist)[1:]) & (lh[1:] > 0)) + 1
        victim = [v for v in comm.allgather_obj(int(whole[0]) if len(whole) else None) if v is not None][0]
        stale = np.array(r.hist, copy=True)
        stale[victim] -= 1
        try:
            distributed.calcPerSegmentStatsDistributed(eng, comm, stale, ENTRIES[0][0], ENTRIES[0][1], imgNullVal=NULLS[0])
        except tilingstats.PyShepSegStatsError as e:
            assert '1 segment ids have more pixels' in str(e), e
            sys.stderr.write('rank %d, %s: %s\n' % (comm.rank, STALE_HISTOGRAM, e))
        else:
            raise AssertionError('%s did not raise' % STALE_HISTOGRAM)
        # nobody is stranded in a collective: the next calls work
        distributed.calcPerSegmentStatsDistributed(eng, comm, r.hist, ENTRIES[0][0], ENTRIES[0][1], imgNullVal=NULLS[0])
        distributed.calcPerSegmentStatsDistributedBands(eng, comm, r.hist, ENTRIES, imgNullVal=NULLS)
        comm.close()
        return
    info = {}
    (ic, fc, fast) = distributed.calcPerSegmentStatsDistributedBands(eng, comm, r.hist, ENTRIES, imgNullVal=NULLS,
                                                                     info=info)
    out = dict(ic=ic, fc=fc, fast=fast, straddlers=info['straddlers'], straddler_pixels=info['straddler_pixels'],
               bands=info['bands'], exchange_bytes=info['exchange_bytes'], path=info['path'])
    for (k, (b, sel)) in enumerate(ENTRIES):
        one = {}
        (ic1, fc1, _f) = distributed.calcPerSegmentStatsDistributed(eng, comm, r.hist, b, sel, imgNullVal=NULLS[k],
                                                                    info=one)
        out.update({'ic%d' % k: ic1, 'fc%d' % k: fc1, 'straddlers%d' % k: one['straddlers'],
                    'straddler_pixels%d' % k: one['straddler_pixels']})
    # one entry is no special route: the same columns
    (icS, fcS, _f) = distributed.calcPerSegmentStatsDistributedBands(eng, comm, r.hist, [ENTRIES[1]], imgNullVal=[NULLS[1]])
    out.update(icS=icS, fcS=fcS)
    np.savez(os.path.join(outdir, 'bands%d.npz' % comm.rank), **out)
    np.savez(os.path.join(outdir, 'rank%d.npz' % comm.rank), out=eng.out, outLo=r.outRows[0], outHi=r.outRows[1],
             maxSegId=r.maxSegId, hist=r.hist)
    comm.close()


if __name__ == '__main__':
    main()
