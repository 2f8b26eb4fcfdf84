"""CPU: distributed.spatialHaloPlan, the halo rows of the spatial statistics split by rows over the ranks.
The plan is played out on a raster whose pixels hold their own global row number: every rank sends what its
plan says into its slot of a simulated all-gather, and the halo rows every rank reads back from it must be
exactly the rows a brute-force owner search names."""
import numpy as np
import pytest

from pyshepseg_amd import distributed
from pyshepseg_amd.tilingstats import PyShepSegStatsError


def _owner(ranges, y):
    own = [r for (r, (a, b)) in enumerate(ranges) if a <= y < b]
    assert len(own) == 1
    return own[0]


def _playOut(ranges, nRows, above, below):
    world = len(ranges)
    plans = [distributed.spatialHaloPlan(ranges, r, nRows, above, below) for r in range(world)]
    slot = above + below
    assert all(p['slot'] == slot for p in plans)
    gathered = np.full((world, max(slot, 1)), -1, dtype=np.int64)   # the rows every rank put in its slot
    for (r, (lo, hi)) in enumerate(ranges):
        own = np.arange(lo, hi)
        for (ownRow, slotRow, n) in plans[r]['send']:
            assert n > 0 and 0 <= ownRow and ownRow + n <= hi - lo and 0 <= slotRow and slotRow + n <= slot
            gathered[r, slotRow:slotRow + n] = own[ownRow:ownRow + n]
    for (r, (lo, hi)) in enumerate(ranges):
        p = plans[r]
        if hi == lo:
            assert p['above'] == p['below'] == 0 and not p['recvAbove'] and not p['recvBelow']
            continue
        wantUp = list(range(max(0, lo - above), lo))
        wantDn = list(range(hi, min(nRows, hi + below)))
        assert (p['above'], p['below']) == (len(wantUp), len(wantDn))
        for (key, want) in (('recvAbove', wantUp), ('recvBelow', wantDn)):
            got = np.full(len(want), -1, dtype=np.int64)
            srcOf = np.full(len(want), -1, dtype=np.int64)
            for (dst, src, slotRow, n) in p[key]:
                assert n > 0 and 0 <= dst and dst + n <= len(want) and slotRow + n <= slot
                assert (got[dst:dst + n] == -1).all()                     # every halo row is filled once
                got[dst:dst + n] = gathered[src, slotRow:slotRow + n]
                srcOf[dst:dst + n] = src
            assert got.tolist() == want, (ranges, r, key)
            assert srcOf.tolist() == [_owner(ranges, y) for y in want]
    return plans


def _randomRanges(rng, nRows, world, emptyShards):
    cuts = np.sort(rng.integers(0, nRows + 1, size=world - 1))
    b = [0] + cuts.tolist() + [nRows]
    ranges = [(b[i], b[i + 1]) for i in range(world)]
    if emptyShards:                 # empty shards of a run without tiles read (0, 0), wherever they sit
        ranges = [(0, 0) if a == bb else (a, bb) for (a, bb) in ranges]
    return ranges


@pytest.mark.parametrize('seed', range(40))
def test_halo_plan_random_row_ranges(seed):
    rng = np.random.default_rng(seed)
    nRows = int(rng.integers(1, 60))
    world = int(rng.integers(1, 9))
    ranges = _randomRanges(rng, nRows, world, seed % 2 == 0)
    for (above, below) in ((0, 0), (1, 1), (0, 1), (0, 5), (0, 12), (0, int(rng.integers(1, 256)))):
        _playOut(ranges, nRows, above, below)


@pytest.mark.parametrize('ranges,nRows', [
    ([(0, 5), (5, 6), (6, 8), (8, 30)], 30),              # 1-row and 2-row shards: the halo spans several ranks
    ([(0, 10), (0, 0), (10, 11), (11, 13), (13, 40)], 40),  # an empty shard in the middle
    ([(0, 0), (0, 20)], 20),                              # the first rank empty
    ([(0, 20), (0, 0)], 20),                              # the last rank empty
    ([(0, 3), (3, 4), (4, 5)], 5),                        # maxDist larger than the whole image
])
def test_halo_plan_thin_and_empty_shards(ranges, nRows):
    for (above, below) in ((1, 1), (0, 1), (0, 5), (0, 12), (0, 255)):
        plans = _playOut(ranges, nRows, above, below)
        # the first rank has nothing above, the last nothing below
        first = min(r for (r, (a, b)) in enumerate(ranges) if b > a)
        last = max(r for (r, (a, b)) in enumerate(ranges) if b > a)
        assert plans[first]['above'] == 0 and plans[last]['below'] == 0


def test_halo_plan_refuses_overlapping_rows():
    ranges = [(0, 12), (8, 20)]            # tile sharding: the ranks share output rows
    for (above, below) in ((1, 1), (0, 3)):
        for r in range(2):
            with pytest.raises(PyShepSegStatsError, match='SHEPSEG_SHARD=rows'):
                distributed.spatialHaloPlan(ranges, r, 20, above, below)
    # mean coordinates need no halo: allowed
    p = distributed.spatialHaloPlan(ranges, 1, 20, 0, 0)
    assert p['slot'] == 0 and p['above'] == p['below'] == 0 and not p['send']


def test_halo_plan_refuses_rows_nobody_holds():
    with pytest.raises(PyShepSegStatsError, match='held by no rank'):
        distributed.spatialHaloPlan([(0, 5), (7, 10)], 0, 10, 0, 3)
