"""Helpers of the tests of user-defined spatial statistics on row shards (test_gpu_spatial_userfunc_distributed.py,
dist_worker_spatial_userfunc_gpu.py): an order-sensitive user function and its numpy restatement."""
import numpy as np


def order_hash(pts, imgNullVal, intArr, floatArr, userParam):
    """Order-sensitive: int column 0 = a position-weighted hash of the (x, y, val) sequence, int column 1 = the
    last point's coordinates and the count plus userParam; float columns = the first point's coordinates."""
    x = np.asarray(pts.x, dtype=np.uint64)
    y = np.asarray(pts.y, dtype=np.uint64)
    v = np.asarray(pts.val, dtype=np.int64).astype(np.uint64)
    k = np.arange(1, len(x) + 1, dtype=np.uint64)
    with np.errstate(over='ignore'):
        h = int(np.sum(k * (x * np.uint64(7919) + y * np.uint64(104729) + v * np.uint64(31)), dtype=np.uint64))
    intArr[0] = h % 2147483647
    if len(intArr) > 1:
        intArr[1] = (int(x[-1]) * 131 + int(y[-1]) * 7 + len(x) + int(userParam)) % 2147483647
    floatArr[0] = float(pts.x[0])
    if len(floatArr) > 1:
        floatArr[1] = float(pts.y[0]) + 0.5


def recording(fn, seg, calls):
    """fn, decorated, that also appends seg[y, x] of every call's first point to ``calls``."""
    from pyshepseg_amd import tilingstats as ts

    def f(pts, imgNullVal, intArr, floatArr, userParam):
        calls.append(int(seg[int(pts.y[0]), int(pts.x[0])]))
        fn(pts, imgNullVal, intArr, floatArr, userParam)
    return ts.spatialUserFunc(f)
