"""World-1 cost of the distributed merge against the one-GPU merge, on the same resident labels and the same table.

    python tools/perf_merge_dist.py [--size 16384] [--repeats 5] [--out results.jsonl]

--size x --size labels of 4 x 8-pixel blocks (shp_dev_block_labels, the raster of tools/perf_merge.py) stay in HBM.
Two rules run: the key column id % 5 (mergeSegments) and the distance rule over 3 float64 columns of uniform random
values with maxDistance 0.4 (mergeSimilarSegments).  For each, distributed.deviceMerge with a one-rank communicator
(no collective runs: the rank's forest pairs are its own, every record is a home record) and the one-GPU function run
in turns on the same table, --repeats times each after one untimed call of each; both upload the table again in every
call (the contracted table displaced it), which is no device time.  The results are compared once, array for array.

One JSON line per rule, medians of the device time the library's events measure per step:
  distributed  hook (local hook), pairs (flatten and pair compaction), pairhook (pair hook; nothing to hook at world
               1), renumber, contract (records, first sort and split, second sort and the share table), recode, and
               records / best where the rule has them
  one_gpu      hook, renumber, contract, recode (and records)
  forest_pairs, records_sent, exchange_bytes   what a rank would send
  ratio        the distributed steps' sum over the one-GPU steps' sum"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

BH, BW = 4, 8


class OneRank(object):
    (rank, world, onDevice) = (0, 1, True)

    def allgather_obj(self, obj):
        return [obj]


def median(values):
    return round(statistics.median(values), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyshepseg_amd import distributed, neighbours, tiling, _lib
    n = a.size
    if n % BH or n % BW:
        raise SystemExit('--size must be a multiple of %d' % BW)
    c = _lib.ctx()
    L = c._L
    comm = OneRank()
    d_seg = ctypes.c_void_p()
    c.check(L.shp_dev_alloc(c.handle, n * n * 4, ctypes.byref(d_seg)))
    try:
        Sc = ctypes.c_uint32(0)
        c.check(L.shp_dev_block_labels(c.handle, n, n, BH, BW, d_seg, ctypes.byref(Sc)))
        S = int(Sc.value)
        kept = type('Kept', (), {'outDev': (d_seg.value, n, n, n * n * 4)})()
        share = distributed.deviceNeighbours(c, comm, d_seg.value, n, n, (0, n), S)
        nb = neighbours.findSegmentNeighbours(kept, True, maxSegId=S)
        size = np.full(S + 1, BH * BW, dtype=np.int64)
        size[0] = 0
        rng = np.random.default_rng(1)
        columns = [rng.random(S + 1) for _ in range(3)]
        rules = [('key id % 5', dict(keyColumn=np.arange(S + 1, dtype=np.int64) % 5)),
                 ('distance, 3 columns', dict(distanceColumns=columns, maxDistance=0.4))]
        for (name, rule) in rules:
            (dist, one, info) = ({}, {}, {})
            for rep in range(-1, a.repeats):
                got = distributed.deviceMerge(c, comm, share, distributed.mergeRule(share, segSize=size, **rule), d_seg.value,
                                              n, n, (0, n), info=info)
                if 'distanceColumns' in rule:
                    want = neighbours.mergeSimilarSegments(nb, rule['distanceColumns'], maxDistance=rule['maxDistance'],
                                                           segSize=size, segfile=kept)
                else:
                    want = neighbours.mergeSegments(nb, rule['keyColumn'], segSize=size, segfile=kept)
                if rep < 0:
                    for k in ('recode', 'representative', 'groupSize', 'hist'):
                        assert np.array_equal(getattr(got, k), getattr(want, k)), k
                    for k in ('offsets', 'neighbours', 'borderLengths'):
                        assert np.array_equal(getattr(got.neighbours, k), getattr(want.neighbours, k)), k
                    assert (got.links, got.recordsSorted) == (want.links, want.recordsSorted)
                    rows = np.empty((2, n), dtype=np.uint32)
                    for (i, r) in enumerate((got, want)):
                        c.check(L.shp_dev_download(c.handle, _lib.ptr(rows[i]), ctypes.c_void_p(r.outDev[0] + 4 * n * (n - 1)),
                                                   4 * n))
                    assert np.array_equal(rows[0], rows[1])
                else:
                    for (acc, res) in ((dist, got), (one, want)):
                        for (k, v) in res.stepDeviceMs.items():
                            acc.setdefault(k, []).append(v)
                tiling.freeDeviceOutput(got)
                tiling.freeDeviceOutput(want)
            (sd, so) = (sum(statistics.median(v) for v in dist.values()), sum(statistics.median(v) for v in one.values()))
            line = json.dumps(dict(what='merge world 1', rule=name, rows=n, cols=n, segments=S, entries=len(nb.neighbours),
                                   groups=want.maxSegId, links=want.links, records=want.recordsSorted, runs=a.repeats,
                                   distributed={k: median(v) for (k, v) in dist.items()},
                                   one_gpu={k: median(v) for (k, v) in one.items()},
                                   distributed_sum_ms=round(sd, 3), one_gpu_sum_ms=round(so, 3), ratio=round(sd / so, 3),
                                   forest_pairs=info['forest_pairs'], records_sent=info['records_sent'],
                                   exchange_bytes=info['exchange_bytes']))
            print(line, flush=True)
            if a.out:
                with open(a.out, 'a') as f:
                    f.write(line + '\n')
    finally:
        c.check(L.shp_dev_free(c.handle, d_seg))


if __name__ == '__main__':
    main()
