"""Helpers of tests/test_neighbours_dist_host.py and tests/test_gpu_neighbours_dist.py (no tests here): a numpy model
of how the distributed neighbour table splits its work over the ranks, and the cases both files run.

The model follows the definition, not the kernels.  Rank r holds the image rows cuts[r] .. cuts[r + 1] - 1 and counts
every differing pixel pair whose UPPER pixel lies in them (for an E pair: either pixel), reading one row below its
own (the halo row).  Its distinct (a, b, count), a < b, are its records.  A record whose two ids both lie in the
rank's id share (distributed.idRange) stays home, the others travel to every rank.  Rank r then takes, from all
travelling records (its own among them), those with a or b in its share, adds its home records, sums the counts per
pair and lists (a, b) under row a if a is in the share and under row b if b is; rows ascend."""
import numpy as np

import neighbour_cases as NC
import stats_bands_dist_helpers as H

FIELD_SEED = 7


def field(kind):
    """(seg, S) of stats_bands_dist_helpers.labelField at the seed these tests use"""
    return H.labelField(kind, np.random.default_rng(FIELD_SEED))


def rankRecords(seg, lo, hi, fourConnected):
    """(keys uint64 a << 32 | b ascending, counts int64) of the pairs whose upper pixel lies in rows lo .. hi - 1"""
    own = seg[lo:hi]
    below = seg[lo + 1:hi + 1]                  # (one row shorter than own where the raster ends at hi)
    n = below.shape[0]
    pairs = [(own[:, :-1], own[:, 1:]), (own[:n], below)]
    if not fourConnected:
        pairs += [(own[:n, :-1], below[:, 1:]), (own[:n, 1:], below[:, :-1])]
    p = np.concatenate([x[0].ravel() for x in pairs]).astype(np.uint64)
    q = np.concatenate([x[1].ravel() for x in pairs]).astype(np.uint64)
    keep = (p != q) & (p != 0) & (q != 0)
    (a, b) = (np.minimum(p, q)[keep], np.maximum(p, q)[keep])
    (keys, counts) = np.unique((a << np.uint64(32)) | b, return_counts=True)
    return keys, counts.astype(np.int64)


def endsOf(keys):
    return (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)


def model(seg, cuts, S, fourConnected):
    """What every rank of the distributed table should hold and report.  cuts: world + 1 row boundaries.  Returns a
    dict: 'ranks' = per rank a dict with keys / counts (its records), home (bool per record), records_local,
    records_home, records_sent, records_picked, entries, idRange, offsets, neighbours, borderLengths; 'halo_rows',
    'exchange_bytes', 'seen' = (all distinct pairs' keys, how many ranks hold a record of each)."""
    from pyshepseg_amd import distributed
    world = len(cuts) - 1
    (nRows, nCols) = seg.shape
    ranks = []
    for r in range(world):
        (keys, counts) = rankRecords(seg, cuts[r], cuts[r + 1], fourConnected)
        (lo, hi) = distributed.idRange(r, world, S)
        (a, b) = endsOf(keys)
        home = (a >= lo) & (a < hi) & (b >= lo) & (b < hi)
        ranks.append(dict(keys=keys, counts=counts, home=home, idRange=(lo, hi), records_local=len(keys),
                          records_home=int(home.sum()), records_sent=int((~home).sum())))
    travK = np.concatenate([m['keys'][~m['home']] for m in ranks])
    travC = np.concatenate([m['counts'][~m['home']] for m in ranks])
    (ta, tb) = endsOf(travK)
    for m in ranks:
        (lo, hi) = m['idRange']
        pick = ((ta >= lo) & (ta < hi)) | ((tb >= lo) & (tb < hi))
        m['records_picked'] = int(pick.sum())
        k = np.concatenate([travK[pick], m['keys'][m['home']]])
        c = np.concatenate([travC[pick], m['counts'][m['home']]])
        (u, inv) = np.unique(k, return_inverse=True)
        tot = np.zeros(len(u), dtype=np.int64)
        np.add.at(tot, inv.reshape(-1), c)
        (a, b) = endsOf(u)
        (ina, inb) = ((a >= lo) & (a < hi), (b >= lo) & (b < hi))
        rows = np.concatenate([a[ina], b[inb]])
        nbrs = np.concatenate([b[ina], a[inb]])
        lens = np.concatenate([tot[ina], tot[inb]])
        order = np.lexsort((nbrs, rows))
        offsets = np.zeros(hi - lo + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(np.bincount(rows - lo, minlength=hi - lo))
        m.update(offsets=offsets, neighbours=nbrs[order].astype(np.uint32), borderLengths=lens[order].astype(np.int64),
                 entries=len(order))
    live = [r for r in range(world) if cuts[r + 1] > cuts[r]]
    halo = sum(1 for r in live if cuts[r + 1] < nRows)
    sent = sum(m['records_sent'] for m in ranks)
    (allK, seen) = np.unique(np.concatenate([m['keys'] for m in ranks]), return_counts=True)
    return dict(ranks=ranks, halo_rows=halo, exchange_bytes=16 * sent + (4 * nCols * len(live) if world > 1 else 0),
                seen=(allK, seen))


def assembled(ranks, S):
    """(offsets, neighbours, borderLengths) of the whole table from the ranks' shares, in id order"""
    offsets = np.zeros(S + 2, dtype=np.int64)
    base = 0
    for m in ranks:
        (lo, hi) = m['idRange']
        offsets[lo:hi + 1] = base + m['offsets']
        base += int(m['offsets'][-1])
    return (offsets, np.concatenate([m['neighbours'] for m in ranks]), np.concatenate([m['borderLengths'] for m in ranks]))


def ownersDiffer(keys, world, S):
    """how many of the pairs have ends in different id shares"""
    from pyshepseg_amd import distributed
    bounds = np.array([distributed.idRange(r, world, S)[1] for r in range(world)])
    (a, b) = endsOf(keys)
    return int((np.searchsorted(bounds, a, side='right') != np.searchsorted(bounds, b, side='right')).sum())


def zeros_raster():
    return np.zeros((40, 70), dtype=np.uint32)


def cases():
    """(name, seg, maxSegId, cuts, fourConnected) of every geometry the distributed table is tested on"""
    out = []
    for kind in ('A', 'B'):
        (seg, S) = field(kind)
        for world in (2, 3, 4):
            for four in (True, False):
                out.append(('%s-w%d-%s' % (kind, world, 'four' if four else 'eight'), seg, S, H.cutsOf(world), four))
    (segA, SA) = field('A')
    out.append(('A-empty-rank', segA, SA, [0, 100, 100, 203], True))
    out.append(('A-one-row-rank', segA, SA, [0, 100, 101, 203], False))
    hp = NC.half_planes()
    out.append(('half-planes-on-border', hp, 2, [0, 150, 300], True))
    out.append(('half-planes-off-border', hp, 2, [0, 149, 300], True))
    out.append(('stripes', NC.stripes(), 2, [0, 64, 65, 200, 257], True))
    for (name, seg) in (('hot-segment', NC.hot_segment()), ('hot-segment-top', NC.hot_segment_top())):
        out.append((name, seg, int(seg.max()), [0, 97, 150, 300], True))
    every = NC.every_pixel_its_own()
    out.append(('every-pixel-its-own', every, int(every.max()), [0, 33, 70], False))
    out.append(('wide-ids', NC.wide_ids(), NC.WIDE_MAX, [0, 30, 60, 90], True))
    out.append(('zeros', zeros_raster(), 9, [0, 10, 20, 30, 40], True))
    return out


def assertReach(name, m, S):
    """the condition under which case ``name`` reaches the path it is meant for, on its model m"""
    ranks = m['ranks']
    (keys, seen) = m['seen']
    world = len(ranks)
    rows = [int((np.diff(r['offsets']) > 0).sum()) for r in ranks]
    longest = max([int(np.diff(r['offsets']).max()) for r in ranks if len(r['offsets']) > 1] or [0])
    if name.startswith('A-w') and name.endswith('four'):
        assert len(keys) == 1673
        assert int((seen >= 2).sum()) == {2: 254, 3: 347, 4: 399}[world]
        assert int((seen >= 3).sum()) == {2: 0, 3: 40, 4: 67}[world]       # (at world 4, seven of them by all four)
        if world == 4:
            assert ownersDiffer(keys, 4, S) == 354
    elif name == 'B-w2-four':
        assert (ranks[0]['records_local'], ranks[0]['records_home'], ranks[0]['records_sent']) == (1090, 1090, 0)
    elif name == 'A-empty-rank':
        assert (ranks[1]['records_local'], ranks[1]['records_home'], ranks[1]['records_sent']) == (0, 0, 0)
        assert rows[1] == 78
    elif name == 'A-one-row-rank':
        assert ranks[1]['records_local'] == 40
    elif name == 'half-planes-on-border':
        assert [r['records_local'] for r in ranks] == [1, 0] and m['halo_rows'] == 1
    elif name == 'half-planes-off-border':
        assert [r['records_local'] for r in ranks] == [0, 1]
    elif name == 'stripes':
        assert seen.tolist() == [4]
        assert [r['borderLengths'].tolist() for r in ranks if r['entries']] == [[257 * 299]] * 2      # (every row's 299 E pairs, from all four ranks)
    elif name.startswith('hot-segment'):
        assert longest == 22500 and int((seen == 2).sum()) == 150
        hot = [r for r in ranks if int(np.diff(r['offsets']).max()) == 22500][0]
        assert hot['records_picked'] > 0 and hot['records_home'] > 0
    elif name == 'every-pixel-its-own':
        assert len(keys) == 35802
    elif name == 'wide-ids':
        assert int(endsOf(keys)[1].max()) > 1 << 24 and min(r['entries'] for r in ranks) == 0
    elif name == 'zeros':
        assert len(keys) == 0 and all(not r['offsets'].any() for r in ranks) and world > 3


CASE_NAMES = [c[0] for c in cases()]


def caseByName(name):
    return [c for c in cases() if c[0] == name][0]
