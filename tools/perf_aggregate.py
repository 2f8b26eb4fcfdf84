"""mergeSimilarSegments' link rules and aggregateToGroups at the C5 size: the neighbour table of a 40000 x 40000 raster
of 4 x 8-pixel blocks (50 M segments, 199.97 M entries: the raster of tools/perf_merge.py), step by step.

    python tools/perf_aggregate.py [--size 40000] [--repeats 3] [--out results.jsonl]

Every figure is the median of --repeats calls after one untimed call, in device ms from the library's events unless
it says wall (one JSON line):
  key_hook_ms                 the hook of mergeSegments under the keys id % 5, on the same resident table
  dist{1,3,6}_hook_ms         the hook under the distance rule with 1, 3 and 6 float64 columns of uniform random
                              values, maxDistance at the lower quartile of the distances over a sample of entries
  dist{1,3,6}_records_ms      laying the uploaded columns out as one record per id
  mutual3_hook_ms             mutualNearest=True with 3 columns and no threshold: the two best passes and the hook
  *_links, *_groups           what the rule found
  members_resident_ms         the member list from the groups a key merge just left on the device (5000 groups of
                              10 000 ids); members_uploaded_ms: from an uploaded recode (the sizes counted as well)
  members_dist3_ms            the same for the groups of the 3-column distance merge (many small groups)
  agg_{key,dist3}_ms, agg_{key,dist3}_weighted_ms
                              one float64 column, all seven statistics, without and with weights
  bincount_wall_ms            numpy on the host for the weighted mean of the same column: two numpy.bincount calls
  *_gb, *_hbm_fraction        the bytes the step must move (below) and that over the device time as a fraction of 8 TB/s
Bytes: a hook = the table (8 B per row, 12 B per entry) + two gathered records of 8 C bytes per entry a < b; the mutual
rule reads the table three times and gathers two records for EVERY entry in each of its two best passes, plus 12 B per
row of best values; records = 16 C bytes per id; members = per id 4 B of recode in, and per 8-bit pass of the sort 8 B
in and 8 B out, then 8 B per member to copy the ids; aggregate = 20 B per member for the weights by entry, 20 B per
member read by the reduction and 8 B gathered, 56 B per group out.
Checked before anything is timed: the distance rule's groups on a 2000 x 2000 corner of the same raster equal the
numpy model of tests/similar_cases.py, and the aggregated weighted mean equals numpy.bincount's to 1e-12."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

BH, BW = 4, 8
HBM_PEAK = 8.0e12


class ResidentLabels(object):
    def __init__(self, ptr, nrows, ncols):
        self.outDev = (ptr, nrows, ncols, nrows * ncols * 4)


def median(values):
    return round(statistics.median(values), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=40000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, 'tests'))
    from pyshepseg_amd import neighbours, _lib
    n = a.size
    if n % BH or n % BW:
        raise SystemExit('--size must be a multiple of %d' % BW)
    c = _lib.ctx()
    L = c._L
    d_seg = ctypes.c_void_p()
    c.check(L.shp_dev_alloc(c.handle, n * n * 4, ctypes.byref(d_seg)))
    try:
        Sc = ctypes.c_uint32(0)
        c.check(L.shp_dev_block_labels(c.handle, n, n, BH, BW, d_seg, ctypes.byref(Sc)))
        S = Sc.value
        rng = np.random.default_rng(1)
        columns = [rng.random(S + 1) for _ in range(6)]
        size = np.full(S + 1, BH * BW, dtype=np.int64)
        size[0] = 0

        # ---- checked once, on a corner small enough for the numpy model ----
        import neighbour_cases as nc
        import similar_cases as sc
        m = min(n, 2000)
        corner = np.empty((m, n), dtype=np.uint32)
        c.check(L.shp_dev_download(c.handle, _lib.ptr(corner), d_seg, corner.nbytes))
        corner = np.ascontiguousarray(corner[:, :m])
        (_u, corner) = np.unique(corner, return_inverse=True)
        corner = (corner.reshape(m, m) + 1).astype(np.uint32)
        Sk = int(corner.max())
        nbk = neighbours.findSegmentNeighbours(corner, True, maxSegId=Sk)
        small = [col[:Sk + 1] for col in columns[:3]]
        for rule in (dict(maxDistance=0.4), dict(mutualNearest=True)):
            got = neighbours.mergeSimilarSegments(nbk, small, **rule)
            want = sc.reference_similar(nc.reference_neighbours(corner, True, Sk), small, **rule)
            assert np.array_equal(got.recode, want.recode) and got.links == want.links, rule
        wk = rng.integers(1, 50, size=Sk + 1).astype(np.int64)
        agg = neighbours.aggregateToGroups(got, [(small[0], [('wm', 'weightedmean')])], weights=wk)
        ref = np.bincount(got.recode, weights=small[0] * wk)[1:] / np.bincount(got.recode, weights=wk)[1:]
        assert np.allclose(agg['wm'][1:], ref, rtol=1e-12, atol=0)
        print('the corner of %d segments: groups and weighted means as numpy has them' % Sk, flush=True)

        t = time.perf_counter()
        nb = neighbours.findSegmentNeighbours(ResidentLabels(d_seg.value, n, n), True, maxSegId=S)
        nent = len(nb.neighbours)
        half = nent // 2
        print('%d segments, %d entries; table in %.2f s (%.1f ms on the device)' % (
            S, nent, time.perf_counter() - t, nb.deviceMs), flush=True)
        assert neighbours.residentTableSerial() == nb.residentSerial
        table = 8.0 * (S + 2) + 12.0 * nent
        line = dict(size=n, segments=S, entries=nent, runs=a.repeats)

        def put(name, ms, nbytes):
            line[name + '_ms'] = median(ms)
            line[name + '_min_max_ms'] = [round(min(ms), 3), round(max(ms), 3)]
            line[name + '_gb'] = round(nbytes / 1e9, 3)
            line[name + '_hbm_fraction'] = round(nbytes / HBM_PEAK / (statistics.median(ms) / 1e3), 4)

        # ---- the hooks, on the resident table (no contraction: the table stays) ----
        (M, counters, ms3) = (ctypes.c_uint32(0), np.zeros(2, dtype=np.int64), np.zeros(3, dtype=np.float64))
        keys = np.arange(S + 1, dtype=np.int64) % 5

        def key_merge():
            c.check(L.shp_nbr_merge(c.handle, _lib.ptr(keys), S + 1, 0, 0, 1, _lib.ptr(size), ctypes.byref(M),
                                    _lib.ptr(counters), _lib.ptr(ms3)))
            return ms3[0]
        ms = [key_merge() for _rep in range(a.repeats + 1)][1:]
        put('key_hook', ms, table + 32.0 * half)
        (line['key_links'], line['key_groups']) = (int(counters[0]), M.value)

        def distance_merge(C, thr2, mutual):
            ptrs = (ctypes.c_void_p * C)(*[col.ctypes.data for col in columns[:C]])
            c.check(L.shp_nbr_merge_similar(c.handle, ptrs, C, S + 1, 0, 0.0, int(thr2 is not None), thr2 or 0.0, int(mutual),
                                            None, 0, 0, 1, _lib.ptr(size), ctypes.byref(M), _lib.ptr(counters),
                                            _lib.ptr(ms3)))
            return (ms3[0], ms3[2])
        sample = rng.integers(0, nent, size=200000)
        rows = np.searchsorted(nb.offsets, sample, side='right') - 1
        thr = {}
        for C in (1, 3, 6):
            d2 = sc.distance2(columns[:C], rows, nb.neighbours[sample].astype(np.int64))
            thr[C] = float(np.quantile(d2, 0.25))
            got = [distance_merge(C, thr[C], False) for _rep in range(a.repeats + 1)][1:]
            put('dist%d_hook' % C, [g[0] for g in got], table + 16.0 * C * half)
            put('dist%d_records' % C, [g[1] for g in got], 16.0 * C * (S + 1))
            (line['dist%d_links' % C], line['dist%d_groups' % C]) = (int(counters[0]), M.value)
        got = [distance_merge(3, None, True) for _rep in range(a.repeats + 1)][1:]
        put('mutual3_hook', [g[0] for g in got], 3.0 * table + 2.0 * 48.0 * nent + 48.0 * half + 12.0 * (S + 1))
        (line['mutual3_links'], line['mutual3_groups']) = (int(counters[0]), M.value)
        print(json.dumps(line), flush=True)

        # ---- the member list and the aggregation ----
        (serial, nmem, msb) = (ctypes.c_uint64(0), ctypes.c_int64(0), ctypes.c_double(0))

        def build(recode=None, groups=0):
            c.check(L.shp_nbr_members_build(c.handle, None if recode is None else _lib.ptr(recode),
                                            0 if recode is None else len(recode), groups, ctypes.byref(serial),
                                            ctypes.byref(nmem), ctypes.byref(msb)))
            return msb.value

        def members_bytes(groups):
            passes = max(1, -(-int(groups).bit_length() // 8))
            return (4.0 + 16.0 * passes) * (S + 1) + 8.0 * S
        column = columns[0]
        weights = size
        for (name, merge) in (('dist3', lambda: distance_merge(3, thr[3], False)), ('key', key_merge)):
            ms = []
            for _rep in range(a.repeats + 1):
                merge()
                ms.append(build())
            put('members_resident' if name == 'key' else 'members_dist3', ms[1:], members_bytes(M.value))
            res = neighbours.MergedSegments()
            (res.recode, res.maxSegId) = (np.empty(S + 1, dtype=np.uint32), M.value)
            c.check(L.shp_nbr_merge_groups(c.handle, _lib.ptr(res.recode), None, None, None))
            (res.groupsSerial, res._groupsCtx) = (neighbours._groupSerials(c)[0], c.handle.value)
            for (tag, w) in (('', None), ('_weighted', weights)):
                ms = []
                for _rep in range(a.repeats + 1):
                    out = neighbours.aggregateToGroups(res, [(column, [(s, s) for s in neighbours.AGGREGATE_STATS])], weights=w)
                    assert res.aggregateTimings['uploaded'] is False and res.aggregateTimings['built'] is False
                    ms.append(res.aggregateTimings['deviceMs'])
                put('agg_%s%s' % (name, tag), ms[1:], 48.0 * S + 56.0 * (M.value + 1))
            assert out['count'].sum() == S and out['weight'].sum() == size.sum()
        ms = [build(res.recode, res.maxSegId) for _rep in range(a.repeats + 1)][1:]
        put('members_uploaded', ms, members_bytes(res.maxSegId) + 4.0 * (S + 1))
        wall = []
        wf = weights.astype(np.float64)
        for _rep in range(a.repeats + 1):
            t = time.perf_counter()
            with np.errstate(invalid='ignore'):             # (row 0: no weight)
                ref = np.bincount(res.recode, weights=column * wf) / np.bincount(res.recode, weights=wf)
            wall.append((time.perf_counter() - t) * 1e3)
        line['bincount_wall_ms'] = median(wall[1:])
        assert np.allclose(out['weightedmean'][1:], ref[1:], rtol=1e-9, atol=0)
        line = json.dumps(line)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    finally:
        if d_seg.value:
            c.check(L.shp_dev_free(c.handle, d_seg))


if __name__ == '__main__':
    main()
