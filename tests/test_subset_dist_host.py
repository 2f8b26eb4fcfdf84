"""CPU: the host logic of distributed.subsetImageDistributed -- which window rows a rank holds, the refusal of
overlapping output rows (on every rank, before anything touches a GPU), and the argument checks and RAT recode
that subset.subsetImage and the distributed entry point share."""
import threading

import numpy as np
import pytest


@pytest.mark.parametrize('rr,tly,ys,want', [
    ((0, 10), 20, 30, (0, 0)),           # shard before the window
    ((0, 20), 20, 30, (0, 0)),           # ... ending where it starts
    ((25, 35), 20, 30, (5, 15)),         # inside
    ((10, 30), 20, 30, (0, 10)),         # across its top
    ((40, 70), 20, 30, (20, 30)),        # across its bottom
    ((0, 100), 20, 30, (0, 30)),         # the whole window
    ((50, 60), 20, 30, (30, 30)),        # after it
    ((70, 90), 20, 30, (30, 30)),
    ((30, 30), 20, 30, (10, 10)),        # empty shard
    ((0, 0), 0, 5, (0, 0)),
    ((3, 4), 3, 1, (0, 1)),              # one row, one-row window
])
def test_subset_held_rows(rr, tly, ys, want):
    from pyshepseg_amd import distributed
    assert distributed.subsetHeldRows(rr, tly, ys) == want


def test_subset_held_rows_brute_force():
    """random shards and windows: (a, b) is exactly the set of window rows whose image row the shard holds, and
    the shards of a row partition cover the window once"""
    from pyshepseg_amd import distributed
    rng = np.random.default_rng(4)
    for _ in range(400):
        n = int(rng.integers(1, 40))
        cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 5))))
        bounds = [0] + cuts.tolist() + [n]
        tly = int(rng.integers(0, n))
        ys = int(rng.integers(0, n - tly + 1))
        cover = np.zeros(ys, dtype=int)
        for (lo, hi) in zip(bounds, bounds[1:]):
            (a, b) = distributed.subsetHeldRows((lo, hi), tly, ys)
            assert 0 <= a <= b <= ys
            want = [r for r in range(ys) if lo <= tly + r < hi]
            assert list(range(a, b)) == want, (lo, hi, tly, ys)
            cover[a:b] += 1
        assert (cover == 1).all()


def test_disjoint_rows_error():
    from pyshepseg_amd import distributed
    assert distributed.disjointRowsError([(0, 10), (10, 20), (20, 20), (0, 0)], 'x') is None
    assert distributed.disjointRowsError([(10, 20), (0, 10)], 'x') is None
    msg = distributed.disjointRowsError([(0, 12), (10, 20)], 'subsetImageDistributed')
    assert 'overlap' in msg and 'SHEPSEG_SHARD=rows' in msg and '0..12' in msg
    # an empty shard inside another's rows is no overlap
    assert distributed.disjointRowsError([(0, 20), (5, 5)], 'x') is None


class _ObjComm(object):
    """`world` threads: allgather_obj only (the collectives deviceSubset makes before it needs a device)"""
    def __init__(self, rank, world, sh):
        (self.rank, self.world, self.sh) = (rank, world, sh)

    def allgather_obj(self, v):
        self.sh['bar'].wait()
        self.sh['slots'][self.rank] = v
        self.sh['bar'].wait()
        out = list(self.sh['slots'])
        self.sh['bar'].wait()
        return out


def _everyRank(ranges, **kw):
    from pyshepseg_amd import distributed
    world = len(ranges)
    sh = {'bar': threading.Barrier(world, timeout=30), 'slots': [None] * world}
    errors = [None] * world

    def rank(r):
        try:
            distributed.deviceSubset(None, _ObjComm(r, world, sh), 0, kw.get('nRows'), 40, ranges[r], 99,
                                     *kw['win'], mask=kw.get('mask'), tileSize=kw.get('tileSize'))
        except BaseException as e:      # noqa: B902
            errors[r] = e
    th = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(60)
    assert not any(t.is_alive() for t in th)
    return errors


@pytest.mark.parametrize('ranges,kw,match', [
    ([(0, 12), (10, 30)], dict(win=(0, 0, 5, 5)), 'disjoint output rows'),
    ([(0, 15), (15, 30)], dict(win=(0, 20, 10, 11)), 'not within input image'),
    ([(0, 15), (15, 30)], dict(win=(35, 0, 6, 10)), 'not within input image'),
    ([(0, 15), (15, 30)], dict(win=(0, 0, 6, 10), nRows=8), 'not within input image'),
    ([(0, 15), (15, 30)], dict(win=(0, 0, 6, 10), mask=np.ones((10, 7), np.uint8)), 'mask should match'),
    ([(0, 15), (15, 30), (30, 30)], dict(win=(0, 0, 6, 10), tileSize=0), 'tileSize must be positive'),
])
def test_device_subset_refuses_on_every_rank(ranges, kw, match):
    """refusals that need no device raise the same error on every rank, none left waiting in a collective"""
    from pyshepseg_amd import subset
    errors = _everyRank(ranges, **kw)
    for e in errors:
        assert isinstance(e, subset.PyShepSegSubsetError), errors
        assert match in str(e)
    assert len({str(e) for e in errors}) == 1


def test_shared_checks():
    from pyshepseg_amd import subset
    subset.checkWindow(50, 60, 10, 10, 50, 40)
    for win in ((10, 10, 51, 40), (10, 10, 50, 41), (-1, 0, 5, 5), (0, -1, 5, 5)):
        with pytest.raises(subset.PyShepSegSubsetError, match='not within input image'):
            subset.checkWindow(50, 60, *win)
    assert subset.loadMask(None, 4, 3) is None
    m = subset.loadMask(np.array([[0, 2, 0, 1], [5, 0, 0, 0], [1, 1, 1, 1]], dtype=np.int16), 4, 3)
    assert m.dtype == np.uint8 and m.flags.c_contiguous
    assert m.tolist() == [[0, 1, 0, 1], [1, 0, 0, 0], [1, 1, 1, 1]]
    with pytest.raises(subset.PyShepSegSubsetError, match='mask should match'):
        subset.loadMask(np.ones((4, 3)), 4, 3)
    subset.checkOutname('x.npy')
    for bad in ('x.tif', 3):
        with pytest.raises(subset.PyShepSegSubsetError, match='outname'):
            subset.checkOutname(bad)


def test_recode_columns():
    """the RAT of the subset: input columns gathered through origSegIds with row 0 = 0, 'Histogram' as float64,
    origSegIdColName as int32 -- the columns subsetImage documents (subset.py:196-266)"""
    from pyshepseg_amd import subset
    orig = np.array([0, 7, 2, 5], dtype=np.uint32)
    hist = np.array([0, 10, 3, 1], dtype=np.uint32)
    v = np.arange(8, dtype=np.float64) * 1.5 + 1
    k = np.arange(100, 108, dtype=np.int32)
    cols = subset.recodeColumns(orig, hist, {'v': v, 'k': k}, 'orig')
    assert list(cols) == ['v', 'k', 'Histogram', 'orig']
    assert cols['v'].tolist() == [0, 11.5, 4.0, 8.5] and cols['v'].dtype == np.float64
    assert cols['k'].tolist() == [0, 107, 102, 105] and cols['k'].dtype == np.int32
    assert cols['Histogram'].dtype == np.float64 and cols['Histogram'].tolist() == [0, 10, 3, 1]
    assert cols['orig'].dtype == np.int32 and cols['orig'].tolist() == [0, 7, 2, 5]
    assert v[1] == 2.5                                   # the input columns are not written
    assert list(subset.recodeColumns(orig, hist, None, None)) == ['Histogram']
    with pytest.raises(subset.PyShepSegSubsetError, match="'v' has 7 rows, segment id 7 needs more"):
        subset.recodeColumns(orig, hist, {'v': v[:7]}, None)
