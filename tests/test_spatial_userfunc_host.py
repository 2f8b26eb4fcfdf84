"""CPU: the host side of user-defined spatial statistics -- the numpy bounding-box helpers, the batch planner of
iterSegmentPoints and the per-segment callback driver, fed with batches built by numpy."""
import numpy as np
import pytest

import segpoints_helpers as H


def _loop_tile(pts, fill, mask):
    xmin, xmax = min(int(p.x) for p in pts), max(int(p.x) for p in pts)
    ymin, ymax = min(int(p.y) for p in pts), max(int(p.y) for p in pts)
    out = np.full((ymax - ymin + 1, xmax - xmin + 1), 0 if mask else fill,
                  dtype=np.uint8 if mask else np.int64)
    for p in pts:
        out[int(p.y) - ymin, int(p.x) - xmin] = 1 if mask else p.val
    return out


@pytest.mark.parametrize('seed', range(4))
def test_convert_points_match_loops(seed):
    from pyshepseg_amd import tilingstats as ts
    rng = np.random.RandomState(seed)
    n = rng.randint(1, 60)
    cells = rng.choice(40 * 30, size=n, replace=False)
    pts = H.as_points(100 + cells % 40, 2000 + cells // 40, rng.randint(-5000, 5000, size=n))
    got = ts.convertPtsInto2DArray(pts, -9)
    assert got.dtype == np.int64 and np.array_equal(got, _loop_tile(pts, -9, False))
    got = ts.convertPtsInto2DMaskArray(pts, -9)
    assert got.dtype == np.uint8 and np.array_equal(got, _loop_tile(pts, -9, True))
    one = pts[3 % n:3 % n + 1]
    assert np.array_equal(ts.convertPtsInto2DArray(one, 0), [[one.val[0]]])


@pytest.mark.parametrize('budget', [1, 5, 17, 1000])
def test_plan_batches(budget):
    from pyshepseg_amd import tilingstats as ts
    rng = np.random.RandomState(budget)
    counts = rng.randint(0, 12, size=300)
    counts[rng.rand(300) < 0.3] = 0
    counts[[7, 150, 299]] = [40, 25, 31]                 # larger than most budgets
    ranges = ts.planPointBatches(counts, budget)
    ids = np.concatenate([np.arange(lo, hi) for (lo, hi) in ranges])
    assert np.array_equal(ids, np.arange(1, 300))           # every id once, in order
    for (lo, hi) in ranges:
        pts = counts[lo:hi].sum()
        if pts > budget:
            assert (counts[lo:hi] > 0).sum() == 1 and hi - lo == 1      # an oversize segment alone
        assert hi > lo
    # batches are filled greedily: a batch could not have taken the next id's points as well
    for (a, b) in zip(ranges[:-1], ranges[1:]):
        assert counts[a[0]:a[1]].sum() + counts[b[0]] > budget or counts[a[0]:a[1]].sum() > budget
    assert ts.planPointBatches(np.zeros(1, np.int64), 10) == []
    assert ts.planPointBatches(np.zeros(4, np.int64), 10) == [(1, 4)]


def _raster(rng):
    seg = np.kron(rng.permutation(np.arange(1, 21)).reshape(4, 5), np.ones((9, 7), np.uint32)).astype(np.uint32)
    band = rng.randint(1, 200, size=seg.shape).astype(np.int16)
    band[rng.rand(*seg.shape) < 0.2] = -1                  # nodata
    band[seg == 6] = -1                                     # a segment that is all nodata
    seg[seg == 11] = 0                                      # an id without pixels
    return seg, band


def test_run_user_func_driver():
    from pyshepseg_amd import tilingstats as ts
    rng = np.random.RandomState(3)
    (seg, band) = _raster(rng)
    S = 23                                                  # ids 21..23 have no pixels either
    calls = []

    def fn(pts, nullv, intArr, floatArr, prm):
        assert nullv == -1 and prm == 'p'
        assert intArr.dtype == np.int32 and floatArr.dtype == np.float64
        assert (intArr == -77).all() and (floatArr == -77).all()       # refilled before every call
        assert len(pts) > 0 and not pts.flags.writeable
        calls.append(int(np.unique(seg[pts.y, pts.x])[0]))
        intArr[0] = int(pts.val.sum())
        intArr[1] = 2 ** 31 - 1 - len(pts)
        floatArr[0] = 1.0 / 3.0 + len(pts)                  # float64 -> float32 rounding in the column
    for ranges in ([(1, S + 1)], ts.planPointBatches(np.bincount(seg.ravel(), minlength=S + 1), 40)):
        calls.clear()
        batches = H.numpy_batches(seg, band, -1, 5, ranges, max_seg_id=S)
        ic, fc = ts.runUserFunc(batches, S + 1, fn, 'p', -1, 2, 2, missingStatsValue=-77)
        assert ic.dtype == np.int64 and fc.dtype == np.float32 and ic.shape == (2, S + 1) and fc.shape == (2, S + 1)
        valid = (band != -1) & (seg != 0)
        want_ids = sorted(set(seg[valid].tolist()))
        assert calls == want_ids                            # ascending, all-nodata / empty ids not called
        assert 6 not in calls and 11 not in calls
        for s in range(S + 1):
            if s == 0:
                assert (ic[:, 0] == 0).all() and (fc[:, 0] == 0).all()
            elif s in want_ids:
                m = valid & (seg == s)
                assert ic[0, s] == band[m].astype(np.int64).sum()
                assert ic[1, s] == 2 ** 31 - 1 - m.sum()
                assert fc[0, s] == np.float32(1.0 / 3.0 + m.sum())
                assert fc[1, s] == -77                      # a column the function leaves alone
            else:
                assert (ic[:, s] == -77).all() and (fc[:, s] == -77).all()


def test_run_user_func_exception_propagates():
    from pyshepseg_amd import tilingstats as ts
    (seg, band) = _raster(np.random.RandomState(5))

    class Boom(Exception):
        pass

    def fn(pts, nullv, intArr, floatArr, prm):
        raise Boom('from the callback')
    with pytest.raises(Boom, match='from the callback'):
        ts.runUserFunc(H.numpy_batches(seg, band, -1, 1024, [(1, 21)]), 21, fn, None, -1, 1, 0)


def test_visit_order_restatement():
    """The numpy restatement used by the GPU tests: row-major inside a tile, tiles row-major."""
    seg = np.ones((5, 7), np.uint32)
    band = np.arange(35, dtype=np.int32).reshape(5, 7)
    (_ids, x, y, _v) = H.visit_points(seg, band, None, 3)
    order = list(zip(y.tolist(), x.tolist()))
    assert order[:9] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]
    assert order[9:12] == [(0, 3), (0, 4), (0, 5)]
    assert order[18:21] == [(0, 6), (1, 6), (2, 6)]
    assert order[21:24] == [(3, 0), (3, 1), (3, 2)]


def test_user_function_gate():
    """As the reference refuses a userFunc that is not @jit / @njit decorated (tilingstats.py:1330-1331), an
    undecorated callable is refused before anything runs; spatialUserFunc marks a plain Python one, and an
    object that carries numba's `targetoptions` passes as in the reference."""
    from pyshepseg_amd import tilingstats as ts
    seg = np.ones((4, 4), np.uint32)
    img = np.ones((4, 4), np.uint16)

    def plain(pts, nullv, intArr, floatArr, prm):
        pass
    for fn in (plain, lambda *a: None, 'not callable'):
        with pytest.raises(ts.PyShepSegStatsError, match='built-in user functions.*spatialUserFunc'):
            ts.calcPerSegmentSpatialStats(seg, img, [ts.GFT_Real], fn, None, 0)
    assert ts.spatialUserFunc(plain) is plain and ts._isUserFunc(plain)
    wrapped = ts.spatialUserFunc(len)                       # a builtin takes no attributes: wrapped
    assert ts._isUserFunc(wrapped) and wrapped([1, 2]) == 2 and not ts._isUserFunc(len)

    class Dispatcher(object):
        def __init__(self):
            self.targetoptions = {'nopython': True}

        def __call__(self, *args):
            pass
    assert ts._isUserFunc(Dispatcher()) and not ts._isUserFunc(lambda *a: None)
