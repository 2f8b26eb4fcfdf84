"""World-1 cost of the distributed neighbour table against the one-GPU table, on the same resident labels.

    python tools/perf_neighbours_dist.py [--size 16384] [--repeats 5] [--eight]

--size x --size labels of 4 x 8-pixel blocks (shp_dev_block_labels) stay in HBM.  distributed.deviceNeighbours with a
one-rank communicator (no collective runs: every record is a home record) and neighbours.findSegmentNeighbours run
in turns, --repeats times each after one untimed call of each; the two tables are compared once.  One JSON line:
the medians (and min / max) of the device time the library's events measure around the kernels of either path.
Both run k_nbr_patch, the two sorts and a run-length reduction; the distributed path adds the pack and (at world
1 idle) pick kernels, the second sort and reduction of the merge and the two columns."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np


class OneRank(object):
    (rank, world, onDevice) = (0, 1, True)

    def allgather_obj(self, obj):
        return [obj]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--eight', action='store_true')
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyshepseg_amd import distributed, neighbours, _lib
    c = _lib.ctx()
    L = c._L
    n = a.size
    if n % 8:
        raise SystemExit('--size must be a multiple of 8')
    four = not a.eight
    d_seg = ctypes.c_void_p()
    c.check(L.shp_dev_alloc(c.handle, n * n * 4, ctypes.byref(d_seg)))
    try:
        Sc = ctypes.c_uint32(0)
        c.check(L.shp_dev_block_labels(c.handle, n, n, 4, 8, d_seg, ctypes.byref(Sc)))
        S = int(Sc.value)
        kept = type('Kept', (), {'outDev': (d_seg.value, n, n, n * n * 4)})()
        (dist, one) = ([], [])
        for rep in range(-1, a.repeats):
            share = distributed.deviceNeighbours(c, OneRank(), d_seg.value, n, n, (0, n), S, fourConnected=four,
                                                 fetch=rep < 0)
            whole = neighbours.findSegmentNeighbours(kept, fourConnected=four, maxSegId=S)
            if rep < 0:
                assert np.array_equal(share.offsets, whole.offsets) and np.array_equal(share.neighbours, whole.neighbours)
                assert np.array_equal(share.borderLengths, whole.borderLengths)
                assert all(np.array_equal(share.columns[k], whole.columns[k]) for k in whole.columns)
            else:
                dist.append(share.deviceMs)
                one.append(whole.deviceMs)
        (md, mo) = (statistics.median(dist), statistics.median(one))
        print(json.dumps(dict(what='neighbours world 1', rows=n, cols=n, fourConnected=four, segments=S,
                              entries=len(whole.neighbours), records_sorted=whole.recordsSorted, runs=a.repeats,
                              distributed_device_ms=round(md, 3), distributed_min_max=[round(min(dist), 3), round(max(dist), 3)],
                              one_gpu_device_ms=round(mo, 3), one_gpu_min_max=[round(min(one), 3), round(max(one), 3)],
                              ratio=round(md / mo, 3))), flush=True)
    finally:
        c.check(L.shp_dev_free(c.handle, d_seg))


if __name__ == '__main__':
    main()
