"""Helpers of tests/test_shapes_dist_host.py and tests/test_gpu_shapes_dist.py (no tests here): a numpy model of how
the distributed shape table (dist_shapes.deviceShapes) splits its work over the ranks, and the cases both files run.

The model follows the definition, not the kernels.  Rank r holds the image rows cuts[r] .. cuts[r + 1] - 1.  Its table
counts the pixels of those rows alone, with coordinates from the whole raster's origin; a pixel's four sides are judged
in the window of the rank's rows and one row on either side of them, clipped to the raster (the halo rows).  Counts and
sums of the ranks add up (modulo 2^64), extents combine by min / max over the ranks that hold the id.  An id that a rank
holds some but not all pixels of is a straddler there and travels as one record of 96 bytes; the rank whose id share
(distributed.idRange) holds the id folds its records."""
import numpy as np

import neighbour_cases as NC
import neighbours_dist_helpers as D
import shape_cases as SC


def rankTable(seg, lo, hi, S):
    """(counts, sums) as shape_cases.reference_shapes gives them, of the rows lo .. hi - 1 of ``seg`` alone: the sides
    from the window [lo - 1, hi + 1) clipped to the raster, coordinates from the whole raster's origin"""
    n = S + 1
    (a, b) = (max(lo - 1, 0), min(hi + 1, seg.shape[0]))
    win = seg[a:b]
    (differs, outer) = SC._sides(win)
    own = slice(lo - a, max(hi, lo) - a)
    sub = win[own]
    (ys, xs) = np.nonzero(sub)
    lab = sub[ys, xs].astype(np.int64)
    (differs, outer) = (differs[:, own], outer[:, own])
    counts = {'area': np.bincount(lab, minlength=n).astype(np.int64),
              'perimeter': np.bincount(lab, weights=differs.sum(axis=0)[ys, xs], minlength=n).astype(np.int64),
              'outerBorder': np.bincount(lab, weights=outer.sum(axis=0)[ys, xs], minlength=n).astype(np.int64),
              'edgePixels': np.bincount(lab, weights=differs.any(axis=0)[ys, xs], minlength=n).astype(np.int64)}
    r = ys.astype(np.int64) + lo
    c = xs.astype(np.int64)
    big = np.iinfo(np.int64).max
    for (name, v, at, init) in (('rowMin', r, np.minimum.at, big), ('rowMax', r, np.maximum.at, -1),
                                ('colMin', c, np.minimum.at, big), ('colMax', c, np.maximum.at, -1)):
        col = np.full(n, init, dtype=np.int64)
        at(col, lab, v)
        col[counts['area'] == 0] = 0
        counts[name] = col
    (ru, cu) = (r.astype(np.uint64), c.astype(np.uint64))
    sums = {}
    for (name, v) in (('sumRow', ru), ('sumCol', cu), ('sumRowRow', ru * ru), ('sumColCol', cu * cu), ('sumRowCol', ru * cu)):
        col = np.zeros(n, dtype=np.uint64)
        np.add.at(col, lab, v)
        sums[name] = col
    return ({k: counts[k] for k in SC.COUNTS}, sums)


def combine(tables):
    """the ranks' (counts, sums) as the exchange combines them: counts and sums add (the sums modulo 2^64, uint64's
    wrap), extents are the min / max over the ranks that hold the id"""
    n = len(tables[0][0]['area'])
    counts = {k: np.zeros(n, dtype=np.int64) for k in ('area', 'perimeter', 'outerBorder', 'edgePixels')}
    sums = {k: np.zeros(n, dtype=np.uint64) for k in SC.SUMS}
    big = np.iinfo(np.int64).max
    ext = {'rowMin': np.full(n, big), 'rowMax': np.full(n, -1), 'colMin': np.full(n, big), 'colMax': np.full(n, -1)}
    for (cn, sm) in tables:
        held = cn['area'] > 0
        for k in counts:
            counts[k] = counts[k] + cn[k]
        for k in sums:
            sums[k] = sums[k] + sm[k]
        for k in ext:
            pick = np.minimum if k.endswith('Min') else np.maximum
            ext[k] = np.where(held, pick(ext[k], cn[k]), ext[k])
    for k in ext:
        counts[k] = np.where(counts['area'] > 0, ext[k], 0).astype(np.int64)
    return ({k: counts[k] for k in SC.COUNTS}, sums)


def model(seg, cuts, S):
    """What every rank of the distributed shape table should report.  cuts: world + 1 row boundaries.  A dict:
    'areas' int64 (world, S + 1), 'hist' their sum, 'strad' bool (world, S + 1): the id is a straddler on that rank,
    'records' per rank, 'picked' records folded per share, 'folded' distinct ids per share, 'straddlers',
    'holders' int (S + 1,): ranks that hold pixels of the id, 'ownerless': straddlers whose id-share owner holds none
    of their pixels, 'halo_rows', 'exchange_bytes', 'info' = the ``info`` dictionary of every rank"""
    from pyshepseg_amd import dist_shapes, distributed
    recordBytes = dist_shapes.SHAPE_RECORD_BYTES
    world = len(cuts) - 1
    (nRows, nCols) = seg.shape
    areas =np.stack([np.bincount(seg[cuts[r]:cuts[r + 1]].ravel().astype(np.int64), minlength=S + 1)[:S + 1]
                      for r in range(world)]).astype(np.int64)
    areas[:, 0] = 0
    hist = areas.sum(axis=0)
    strad = (areas > 0) & (areas < hist[None, :])
    records = [int(x) for x in strad.sum(axis=1)]
    perId = strad.sum(axis=0)
    shares = [distributed.idRange(r, world, S) for r in range(world)]
    picked = [int(perId[lo:hi].sum()) for (lo, hi) in shares]
    folded = [int((perId[lo:hi] > 0).sum()) for (lo, hi) in shares]
    owner = np.zeros(S + 1, dtype=np.int64)
    for (r, (lo, hi)) in enumerate(shares):
        owner[lo:hi] = r
    ids = np.flatnonzero(perId > 0)
    live = [r for r in range(world) if cuts[r + 1] > cuts[r]]
    halo = sum(int(cuts[r] > 0) + int(cuts[r + 1] < nRows) for r in live)
    xbytes = recordBytes * sum(records) + (8 * nCols * len(live) if world > 1 else 0)
    info = [dict(halo_rows=halo, records_sent=records[r], records_picked=picked[r], straddlers=len(ids), exchange_bytes=xbytes)
            for r in range(world)]
    return dict(areas=areas, hist=hist, strad=strad, records=records, picked=picked, folded=folded, straddlers=len(ids),
                holders=(areas > 0).sum(axis=0), ownerless=int((areas[owner[ids], ids] == 0).sum()), halo_rows=halo,
                exchange_bytes=xbytes, info=info)


def five_kinds():
    """(seg, S, cuts): uniform labels 0 .. 5 under S = 8 -- fields A and B have no different non-zero pair across a
    cut.  Every cut lies on or next to a 32-row patch edge and sees all five kinds of pair; ids 1 - 5 are on all four
    ranks and the last rank's id share [6, 9) is empty"""
    return NC.random_labels((130, 200), 5, 11), 8, [0, 32, 64, 65, 130]


def pairKinds(seg, row):
    """the vertical pairs between image rows row - 1 and row: [equal non-zero, different non-zero, zero below, zero
    above, both zero]"""
    (up, dn) = (seg[row - 1].astype(np.int64), seg[row].astype(np.int64))
    return [int(((up == dn) & (up != 0)).sum()), int(((up != dn) & (up != 0) & (dn != 0)).sum()),
            int(((up != 0) & (dn == 0)).sum()), int(((up == 0) & (dn != 0)).sum()), int(((up == 0) & (dn == 0)).sum())]


# (name in neighbours_dist_helpers.cases() -- connectivity plays no part here -- or 'five-kinds')
GPU_CASES = ['A-w2-four', 'A-w3-four', 'A-w4-four', 'B-w4-four', 'A-empty-rank', 'A-one-row-rank', 'half-planes-on-border',
             'half-planes-off-border', 'stripes', 'hot-segment', 'every-pixel-its-own', 'zeros', 'five-kinds']


def caseByName(name):
    """(seg, S, cuts)"""
    if name == 'five-kinds':
        return five_kinds()
    (_n, seg, S, cuts, _four) = D.caseByName(name)
    return seg, S, cuts


def hostCases():
    """(name, seg, S, cuts) of every four-connected geometry of neighbours_dist_helpers.cases() bar 'wide-ids' (1.5 GB
    of table per rank for a property the one-GPU test pins), and the new raster"""
    out = [(n, seg, S, cuts) for (n, seg, S, cuts, four) in D.cases() if four and n != 'wide-ids']
    out.append(('A-one-row-rank',) + caseByName('A-one-row-rank'))
    out.append(('five-kinds',) + five_kinds())
    return out


def assertReach(name, seg, cuts, S, m):
    """the condition under which case ``name`` reaches the path it is meant for, on its model m"""
    world = len(cuts) - 1
    holders = m['holders']
    sid = np.flatnonzero(m['strad'].any(axis=0))
    whole = [int(((m['areas'][r] > 0) & ~m['strad'][r]).sum()) for r in range(world)]
    if name == 'A-w2-four':
        assert m['straddlers'] == 187
    elif name == 'A-w3-four':
        assert (m['straddlers'], int((holders[sid] == 3).sum()), m['ownerless']) == (195, 140, 21)
        assert m['records'] == [178, 177, 175]
    elif name == 'A-w4-four':
        assert (m['straddlers'], int((holders[sid] >= 3).sum()), m['ownerless']) == (199, 171, 37)
    elif name == 'B-w4-four':
        assert m['straddlers'] == 138 and int(holders.max()) == 2
        assert all(150 <= w <= 200 for w in whole), whole
        assert int((m['hist'][1:] == 0).sum()) == 1058
    elif name == 'A-empty-rank':
        assert m['records'] == [187, 0, 187] and m['ownerless'] == 75
        assert m['halo_rows'] == 2                  # (each from the rank beyond the empty one)
    elif name == 'A-one-row-rank':
        assert m['records'] == [187, 39, 187] and cuts[2] - cuts[1] == 1 and m['halo_rows'] == 4
    elif name == 'half-planes-on-border':
        assert pairKinds(seg, cuts[1]) == [0, 300, 0, 0, 0] and m['straddlers'] == 0 and m['exchange_bytes'] == 8 * 300 * 2
    elif name == 'half-planes-off-border':
        assert pairKinds(seg, cuts[1]) == [300, 0, 0, 0, 0] and m['records'] == [1, 1]
    elif name == 'stripes':
        assert sid.tolist() == [1, 2] and holders[sid].tolist() == [4, 4]
        assert cuts[1] % SC.PATCH_ROWS == 0 and cuts[2] - cuts[1] == 1
    elif name == 'hot-segment':
        assert sid.tolist() == [1] and int(holders[1]) == 3 and sum(whole) == 22500
        assert int((m['hist'][2:] == 1).sum()) == 22500
        assert all(pairKinds(seg, y) == [150, 150, 0, 0, 0] for y in cuts[1:-1])
    elif name == 'every-pixel-its-own':
        assert m['straddlers'] == 0
        for r in range(world):          # either rank's first patches hold more labels than the LDS table has slots
            rows = min(cuts[r + 1] - cuts[r], SC.PATCH_ROWS)
            assert rows * SC.PATCH_COLS > SC.TABLE_SLOTS
    elif name == 'zeros':
        assert not m['hist'].any() and m['exchange_bytes'] == 8 * seg.shape[1] * 4 and world == 4
    elif name == 'five-kinds':
        assert [pairKinds(seg, y) for y in cuts[1:-1]] == [[28, 107, 29, 31, 5], [26, 127, 22, 24, 1], [35, 109, 33, 18, 5]]
        assert sid.tolist() == [1, 2, 3, 4, 5] and holders[sid].tolist() == [4] * 5
        assert m['picked'][3] == 0 and m['folded'][3] == 0
        assert all(y % SC.PATCH_ROWS in (0, 1) for y in cuts[1:-1])
