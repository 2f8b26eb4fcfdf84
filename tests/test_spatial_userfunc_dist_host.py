"""CPU: the host side of user-defined spatial statistics on row shards (distributed.userFuncRowPlan,
clearUnownedRows, userFuncErrorOf): played out over random row shards against a brute-force account of which
rank holds which pixels, every row of the columns has exactly one writer and every id with points exactly one
call, and the ranks' column blocks add up (as int64 words) to the one-process columns."""
import numpy as np
import pytest


def _shards(rng, nr, world):
    cuts = np.sort(rng.integers(0, nr + 1, size=world - 1))
    b = [0] + cuts.tolist() + [nr]
    return [(b[r], b[r + 1]) for r in range(world)]


def _play(seed, world):
    """one raster, its shards, and every rank's plan as deviceSpatialStats computes it"""
    from pyshepseg_amd import distributed
    rng = np.random.default_rng(seed)
    (nr, nc) = (int(rng.integers(1, 30)), int(rng.integers(1, 20)))
    S = int(rng.integers(1, 60))
    seg = rng.integers(0, S + 1, size=(nr, nc))
    seg[:, :2] = S // 2 + 1 if S > 1 else 1          # a segment down the whole raster (crosses every boundary)
    seg = np.minimum(seg, S)
    nodata = rng.random((nr, nc)) < 0.3
    nodata[seg == 1] = True                           # id 1 has no points anywhere
    S += 3                                            # ids nobody holds
    hist = np.bincount(seg.ravel(), minlength=S + 1).astype(np.int64)
    hist[0] = 0
    shards = _shards(rng, nr, world)
    lhs, lps = [], []
    for (a, b) in shards:
        s = seg[a:b]
        lh = np.bincount(s.ravel(), minlength=S + 1)
        lh[0] = 0
        lp = np.bincount(s[~nodata[a:b]].ravel(), minlength=S + 1)
        lp[0] = 0
        lhs.append(lh)
        lps.append(lp)
    strad = [(lh > 0) & (lh < hist) for lh in lhs]
    pointless = np.concatenate([np.flatnonzero(st & (lp == 0)) for (st, lp) in zip(strad, lps)])
    plans = []
    for r in range(world):
        (lo, hi) = distributed.idRange(r, world, S)
        # the records of the share's straddlers, from every rank
        merged = sum(np.where(st, lp, 0) for (st, lp) in zip(strad, lps))[lo:hi]
        plans.append(distributed.userFuncRowPlan(hist, lhs[r], lps[r], (lo, hi), merged, pointless))
    total = np.bincount(seg[~nodata].ravel(), minlength=S + 1)
    total[0] = 0
    anyStrad = np.logical_or.reduce(strad)
    return S, hist, total, plans, anyStrad


@pytest.mark.parametrize('seed', range(40))
@pytest.mark.parametrize('world', [1, 2, 3, 5])
def test_row_plan_one_writer_one_call(seed, world):
    (S, hist, total, plans, anyStrad) = _play(seed * 7 + world, world)
    owners = sum(p[1].astype(int) for p in plans)
    assert (owners[1:] == 1).all()                     # every row but row 0 has exactly one writer
    calls = sum((p[0] > 0).astype(int) for p in plans)
    assert np.array_equal(calls, (total > 0).astype(int))     # every id with points called once, nowhere else
    for p in plans:
        called = p[0] > 0
        assert np.array_equal(p[0][called], total[called])   # with all of its points
        assert not (called & ~p[1]).any()
    assert sum(p[2] for p in plans) == int(np.count_nonzero(anyStrad))


@pytest.mark.parametrize('seed', range(10))
def test_columns_add_up_as_int64_words(seed):
    """runUserFunc's columns on every rank, cleared to the owned rows, summed as the all-reduce sums them (int64
    words of the int block, then the float block): the one-process columns bit for bit"""
    from pyshepseg_amd import distributed
    world = 1 + seed % 4
    (S, hist, total, plans, _s) = _play(100 + seed, world)
    (nInt, nFloat, missing) = (2, 3, -9999)
    ns = S + 1

    def columns(called):
        rng = np.random.default_rng(seed)
        ic = np.full((nInt, ns), missing, np.int64)
        fc = np.full((nFloat, ns), missing, np.float32)
        ic[:, 0] = 0
        fc[:, 0] = 0
        vals_i = rng.integers(-2**31, 2**31, size=(nInt, ns))
        vals_f = rng.standard_normal((nFloat, ns)).astype(np.float32)
        vals_f[:, ::5] = -0.0
        ic[:, called] = vals_i[:, called]
        fc[:, called] = vals_f[:, called]
        return ic, fc
    want = columns(total > 0)
    colWords = ((nInt * 8 + nFloat * 4) * ns + 7) // 8
    acc = np.zeros(colWords, np.int64)
    for (emit, owned, _n) in plans:
        (ic, fc) = columns(emit > 0)
        distributed.clearUnownedRows(ic, fc, owned)
        block = np.zeros(colWords * 8, np.uint8)
        block[:ic.nbytes] = ic.reshape(-1).view(np.uint8)
        block[ic.nbytes:ic.nbytes + fc.nbytes] = fc.reshape(-1).view(np.uint8)
        acc += block.view(np.int64)
    got = acc.view(np.uint8)
    assert np.array_equal(got[:want[0].nbytes].view(np.int64).reshape(nInt, ns), want[0])
    gf = got[want[0].nbytes:want[0].nbytes + want[1].nbytes].view(np.uint32).reshape(nFloat, ns)
    assert np.array_equal(gf, want[1].view(np.uint32))


def test_user_function_error_message():
    from pyshepseg_amd import distributed
    assert distributed.userFuncErrorOf([None, None]) is None
    msg = distributed.userFuncErrorOf([None, ('ZeroDivisionError', 'division by zero'), ('KeyError', '3')])
    assert 'rank 1' in msg and 'ZeroDivisionError' in msg and 'division by zero' in msg


def test_emit_point_batches_order():
    """the double-buffered emission hands the batches over in order, each with its emit's offsets and count"""
    from pyshepseg_amd import tilingstats as ts

    class Buf(object):
        def __init__(self):
            self.p = None
            self.n = None

        def points(self, n):
            return ('pts', self.n, n)
    bufs = [Buf(), Buf()]
    batches = [(1, 4), (4, 5), (5, 9)]

    def emit(lo, hi, offs, buf, n):
        offs[:] = np.arange(hi - lo + 1) * 2
        n.value = 2 * (hi - lo)
    got = list(ts.emitPointBatches(batches, bufs, emit))
    assert [g[0].tolist() for g in got] == [[1, 2, 3], [4], [5, 6, 7, 8]]
    assert [g[2][2] for g in got] == [6, 2, 8]
    assert all(not g[1].flags.writeable for g in got)
