"""The distributed shape path at world 1 against the one-GPU function, on the same resident labels in one process.

    python tools/perf_shapes_dist.py [--sizes 8192,40000] [--repeats 3]

Per size a raster of 4 x 8-pixel blocks (tools/perf_shapes.py's) and one JSON line: the library's device events of
distributed.deviceShapes (a communicator of one rank: no halo, no record, no all-reduce) and of shapes.calcSegmentShapes,
called in turns, --repeats calls each after an untimed one whose columns are compared by bytes."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

import perf_shapes as P


class Alone(object):
    """one rank: the control data comes straight back, no device collective is reached"""
    onDevice = True
    (rank, world) = (0, 1)

    def allgather_obj(self, obj):
        return [obj]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='8192,40000')
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyshepseg_amd import distributed, shapes, _lib
    c = _lib.ctx()
    L = c._L
    for n in [int(x) for x in a.sizes.split(',')]:
        if n % P.BW:
            raise SystemExit('sizes must be multiples of %d' % P.BW)
        d_seg = ctypes.c_void_p()
        c.check(L.shp_dev_alloc(c.handle, n * n * 4, ctypes.byref(d_seg)))
        try:
            Sc = ctypes.c_uint32(0)
            c.check(L.shp_dev_block_labels(c.handle, n, n, P.BH, P.BW, d_seg, ctypes.byref(Sc)))
            S = (n // P.BH) * (n // P.BW)
            hist = np.full(S + 1, P.BH * P.BW, dtype=np.uint32)
            hist[0] = 0
            labels = P.ResidentLabels(d_seg.value, n, n)
            (one, dist, steps) = ([], [], None)
            for rep in range(-1, a.repeats):
                w = shapes.calcSegmentShapes(labels, maxSegId=S)
                d = distributed.deviceShapes(c, Alone(), d_seg.value, n, n, (0, n), S, hist)
                if rep < 0:
                    for k in w.columns:
                        assert w.columns[k].tobytes() == d.columns[k].tobytes(), k
                else:
                    one.append(w.deviceMs)
                    dist.append(d.deviceMs)
                    steps = {k: round(v, 4) for (k, v) in d.timings.items()}
                del w, d
            print(json.dumps(dict(what='blocks', rows=n, cols=n, segments=S, runs=len(one),
                                  distributed_device_ms=round(statistics.median(dist), 3),
                                  distributed_min_ms=round(min(dist), 3), distributed_max_ms=round(max(dist), 3),
                                  one_gpu_device_ms=round(statistics.median(one), 3), one_gpu_min_ms=round(min(one), 3),
                                  one_gpu_max_ms=round(max(one), 3), steps_s=steps)), flush=True)
        finally:
            c.check(L.shp_dev_free(c.handle, d_seg))


if __name__ == '__main__':
    main()
