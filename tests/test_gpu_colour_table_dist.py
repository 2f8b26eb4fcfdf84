"""GPU: colour tables and the RGBA rendering on the row-sharded multi-rank output
(distributed.writeColorTableFromRatColumnsDistributed / deviceColourTable: shp_dcolour_*, shp_colour_pack_dev;
renderColourTableDistributed / deviceRender: shp_colour_render_rows_dev, shp_colour_overview_rects_dev).
Every comparison is np.array_equal on bytes and on the bit patterns of the float64 stretch: against numpy's own
percentile and stretch expression, and against the one-GPU functions of pyshepseg_amd.utils."""
import os

import numpy as np
import pytest

from conftest import ROOT

import dist_cases
import stats_bands_dist_helpers as H

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------
# numpy's side
# ------------------------------------------------------------------------------------------
def _numpyStretch(col):
    """utils.py:216-221 of the reference in numpy: (bytes, (lo, hi))"""
    col = np.asarray(col).astype(np.float64)
    (lo, hi) = (np.percentile(col, 5), np.percentile(col, 95))
    with np.errstate(divide='ignore', invalid='ignore'):
        clr = (255 * ((col - lo) / (hi - lo)).clip(0, 1)).astype(np.uint8)
    return clr, (np.float64(lo), np.float64(hi))


def _ranksOf(n):
    """the ranks (prev, next) of numpy's 5th and 95th percentile in a sorted column of n rows"""
    out = []
    for q in (5, 95):
        prev = int(np.floor((n - 1) * (q / 100.0)))
        out += [prev, min(prev + 1, n - 1)]
    return out


def _shareOf(shares, i):
    return [r for (r, (a, b)) in enumerate(shares) if a <= i < b][0]


def _placeOrderStatistics(col, world):
    """Swap values of a column of DISTINCT values so that its four order statistics (ranks _ranksOf) sit in the
    shares 0, 1, 2, 3 (mod world) -- the multiset, and with it every percentile, stays what it was.  Returns the
    shares that hold them."""
    from pyshepseg_amd import distributed
    n = len(col)
    shares = distributed.colourShares(n, world)
    order = np.argsort(col, kind='stable')
    taken = set()
    for (k, rank) in enumerate(_ranksOf(n)):
        (a, b) = shares[k % world]
        at = int(order[rank])
        target = [i for i in range(a + 1 + k, b) if i not in taken][0]       # (not the first row of a share)
        (col[at], col[target]) = (col[target], col[at])
        order = np.argsort(col, kind='stable')
        taken.add(target)
    order = np.argsort(col, kind='stable')
    return [_shareOf(shares, int(order[rank])) for rank in _ranksOf(n)]


def _columnSets(world, rng):
    """Two sets of (red, green, blue) source columns of 1009 rows, and what numpy counts in them.  Set 0: float64,
    float32 and int64 columns of distinct values around zero whose four order statistics lie in different shares;
    set 1: a constant float64 column, an int64 column of few distinct values (the order statistics tie), a float32
    column with -0.0 and negative values."""
    n = 1009
    f64 = rng.permutation(n).astype(np.float64) * 0.37 - 150.0 + rng.random(n) * 0.01
    f32 = (rng.permutation(n).astype(np.float32) - 400.0) * np.float32(1.5)
    i64 = rng.permutation(n).astype(np.int64) * 1000003 - 5 * 10 ** 8
    facts = {}
    for (name, col) in (('f64', f64), ('f32', f32), ('i64', i64)):
        assert len(np.unique(col)) == n
        held = _placeOrderStatistics(col, world)
        # ---- what the case relies on: the four elements in different shares (as many as there are), and a share
        #      boundary between the rank-prev and the rank-next element of each percentile
        assert len(set(held)) == min(world, 4), (name, held)
        assert held[0] != held[1] and held[2] != held[3], (name, held)
        assert (col < 0).any() and (col > 0).any()
        facts[name] = held
    const = np.full(n, 1234.5, dtype=np.float64)
    ties = rng.integers(-3, 4, size=n).astype(np.int64)
    srt = np.sort(ties)
    (p5, n5, p95, n95) = _ranksOf(n)
    assert srt[p5] == srt[n5] and srt[p95] == srt[n95] and srt[p5] != srt[p95]      # two of them tie, twice
    zeros = (rng.integers(-20, 21, size=n) * 0.25).astype(np.float32)
    zeros[rng.random(n) < 0.2] = np.float32(-0.0)
    assert np.signbit(zeros[zeros == 0]).any() and not np.signbit(zeros[zeros == 0]).all() and (zeros < 0).any()
    return [(f64, f32, i64), (const, ties, zeros)], facts


def _tableBody(cols):
    """what every rank thread does: deviceColourTable, then the packed table is fetched and freed"""
    from pyshepseg_amd import distributed, tiling, _lib

    def body(r, comm, c):
        info = {}
        (columns, stretch, ms, d_table, n) = distributed.deviceColourTable(c, comm, cols[r] if isinstance(cols, dict) else cols,
                                                                           info=info)
        try:
            table = np.empty(n, dtype=np.uint32)
            c.check(c._L.shp_dev_download(c.handle, _lib.ptr(table), d_table, table.nbytes))
        finally:
            tiling._devRelease(c, d_table, n * 4)
        return columns, stretch, ms, table, info
    return body


def _checkTable(result, cols, world, rank):
    from pyshepseg_amd import distributed, utils
    (columns, stretch, ms, table, info) = result
    n = len(cols[0])
    one = utils.writeColorTableFromRatColumns({'r': cols[0], 'g': cols[1], 'b': cols[2]}, 'r', 'g', 'b')
    for (k, name) in enumerate(('Red', 'Green', 'Blue')):
        (clr, lohi) = _numpyStretch(cols[k])
        print('rank %d %s: stretch %r (numpy %r)' % (rank, name, stretch[k], lohi))
        assert columns[name].dtype == np.uint8 and np.array_equal(columns[name], clr), (rank, name)
        assert np.array_equal(np.array(stretch[k], dtype=np.float64).view(np.uint64),
                              np.array(lohi, dtype=np.float64).view(np.uint64)), (rank, name, stretch[k], lohi)
        assert np.array_equal(columns[name], one.columns[name]), (rank, name)
        assert np.array_equal(np.array(stretch[k]).view(np.uint64), np.array(one.stretch[k]).view(np.uint64)), (rank, name)
    assert np.array_equal(columns['Alpha'], np.full(n, 255, dtype=np.uint8))
    want = (columns['Red'].astype(np.uint32) | columns['Green'].astype(np.uint32) << 8 |
            columns['Blue'].astype(np.uint32) << 16 | np.uint32(255) << 24)
    assert np.array_equal(table, want), rank
    assert tuple(info['rows']) == distributed.colourShares(n, world)[rank]
    assert info['exchange_bytes'] == (3 * ((8 * 512 + 1) * 8 * world + n) if world > 1 else 0)
    assert info['deviceMs'] == ms and ms >= 0


# ------------------------------------------------------------------------------------------
# 1. the selection does not depend on the split
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('world', [2, 3, 4])
def test_colour_table_does_not_depend_on_the_split(world):
    """float64, float32 and int64 columns shared over 2, 3 and 4 rank threads of this GPU: bytes and percentiles ==
    numpy's == the one-GPU function's on the whole column, on every rank.  The columns place the four order
    statistics in different shares, tie them, hold negatives and -0.0, and one is constant (_columnSets)."""
    rng = np.random.default_rng(10 + world)
    (sets, facts) = _columnSets(world, rng)
    print('world %d: the order statistics lie in the shares %s' % (world, facts))
    for cols in sets:
        (results, errors) = H.runRankThreads(world, _tableBody(cols))
        assert not any(errors), errors
        for (r, res) in enumerate(results):
            _checkTable(res, cols, world, r)
    (clr, lohi) = _numpyStretch(sets[1][0])
    assert lohi[0] == lohi[1] and not clr.any()              # the constant column: numpy's NaN casts to 0


@pytest.mark.parametrize('n,world', [(3, 4), (1, 3), (2, 2)])
def test_more_ranks_than_rows(n, world):
    """a world larger than the column: ranks with an empty share upload nothing and take part in every collective"""
    from pyshepseg_amd import distributed
    rng = np.random.default_rng(n)
    cols = (rng.normal(size=n), rng.normal(size=n).astype(np.float32), rng.integers(-50, 50, size=n).astype(np.int64))
    shares = distributed.colourShares(n, world)
    assert sum(1 for (a, b) in shares if a == b) == max(world - n, 0)
    (results, errors) = H.runRankThreads(world, _tableBody(cols))
    assert not any(errors), errors
    for (r, res) in enumerate(results):
        _checkTable(res, cols, world, r)


# ------------------------------------------------------------------------------------------
# 2. errors reach every rank
# ------------------------------------------------------------------------------------------
def _errorCases(world):
    from pyshepseg_amd import distributed
    n = 500
    shares = distributed.colourShares(n, world)
    rng = np.random.default_rng(4)
    good = [rng.normal(size=n), rng.normal(size=n).astype(np.float32), rng.integers(-9, 9, size=n).astype(np.int64)]
    cases = []
    for (bad, where) in ((np.nan, world - 1), (np.inf, 0)):
        cols = [c.copy() for c in good]
        cols[1][shares[where][0] + 2] = bad                  # in one rank's share only, and in the second column
        assert sum(1 for (a, b) in shares if not np.isfinite(cols[1][a:b]).all()) == 1
        cases.append((cols, 'column holds a NaN or an infinity'))
    cols = [c.copy() for c in good]
    cols[2][shares[world // 2][1] - 1] = -(1 << 53)
    assert sum(1 for (a, b) in shares if (np.abs(cols[2][a:b]) >= 1 << 53).any()) == 1
    cases.append((cols, 'integer column holds a magnitude of 2^53 or more: not exact in float64'))
    perRank = {r: [c.copy() for c in good] for r in range(world)}
    perRank[world - 1][1] = perRank[world - 1][1][:-1]       # one rank's green column is a row short
    cases.append((perRank, 'the three columns differ in length'))
    perRank = {r: [c[:n - (r == 1)].copy() for c in good] for r in range(world)}    # rank 1: all three a row short
    cases.append((perRank, 'the columns differ in length between the ranks'))
    return cases


@pytest.mark.parametrize('world', [2, 3])
def test_column_errors_raise_on_every_rank(world):
    """a NaN / an infinity in one rank's share only, a 2^53 integer in one share only, unequal lengths on one rank
    and between the ranks: every rank raises PyShepSegUtilsError with the one-GPU wording, and every rank returns"""
    from pyshepseg_amd import utils
    for (cols, wording) in _errorCases(world):
        (results, errors) = H.runRankThreads(world, _tableBody(cols), timeout=120)
        assert results == [None] * world, wording
        for (r, e) in enumerate(errors):
            assert isinstance(e, utils.PyShepSegUtilsError), (wording, r, e)
            assert wording in str(e), (wording, r, e)


# ------------------------------------------------------------------------------------------
# 3. rendering
# ------------------------------------------------------------------------------------------
def _rects(h):
    """two made-up overview rectangles over a block of h rows: every 2nd pixel of every 2nd row, and every 4th
    from pixel (2, 2) on (overviewTable's words)"""
    out = []
    at = 0
    for (lvl, y0, x0) in ((2, 0, 0), (4, 2, 2)):
        (nr, nc) = ((h - y0 + lvl - 1) // lvl if h > y0 else 0, (H.NC - x0 + lvl - 1) // lvl)
        if nr > 0:
            out.append((y0 * H.NC + x0, lvl * H.NC, lvl, nr, nc, at))
            at += nr * nc
    return np.array(out, dtype=np.int64).reshape(-1, 6), at


def _renderBody(seg, cuts, colours, nTable, blockPixels):
    from pyshepseg_amd import distributed, tiling, _lib

    def body(r, comm, c):
        (lo, hi) = (cuts[r], cuts[r + 1])
        ds = H.uploadRows(c, seg[lo:hi]) if hi > lo else None
        d_table = tiling._devAlloc(c, nTable * 4)
        try:
            cols = [np.ascontiguousarray(colours[k][:nTable]) for k in ('Red', 'Green', 'Blue', 'Alpha')]
            c.check(c._L.shp_colour_pack(c.handle, _lib.ptr(cols[0]), _lib.ptr(cols[1]), _lib.ptr(cols[2]),
                                         _lib.ptr(cols[3]), nTable, d_table))
            (rects, npacked) = _rects(hi - lo)
            info = {}
            sunk = []
            res = distributed.deviceRender(c, comm, ds, hi - lo, H.NC, d_table, nTable, rects=rects, npacked=npacked,
                                           blockPixels=blockPixels, info=info)
            res2 = distributed.deviceRender(c, comm, ds, hi - lo, H.NC, d_table, nTable, blockPixels=blockPixels,
                                            sink=lambda y0, y1, rows: sunk.append((y0, y1, rows.copy())))
        finally:
            tiling._devRelease(c, d_table, nTable * 4)
            if ds is not None:
                c.check(c._L.shp_dev_free(c.handle, ds))
        return res, res2, sunk, info
    return body


RENDER_CASES = [pytest.param('A', [0, 61, 203], id='A-w2-uneven'), pytest.param('B', [0, 30, 131, 203], id='B-w3-uneven'),
                pytest.param('A', [0, 100, 100, 203], id='A-w3-rank-without-rows'),
                pytest.param('B', [0, 0, 57, 140, 203], id='B-w4-first-rank-without-rows')]


@pytest.mark.parametrize('field,cuts', RENDER_CASES)
def test_render_rows_of_every_rank(field, cuts):
    """rank threads paint their rows of label fields 'A' and 'B' through a random table: rows ==
    np.stack([R, G, B, A], -1)[seg[lo:hi]], collected or handed to a sink group by group, in blocks of 9 rows (a
    block that is no multiple of four pixels, several blocks per group, a last group that is not full); the
    overview rectangles' colours == the same lookup of the sampled labels"""
    from pyshepseg_amd import distributed, utils
    world = len(cuts) - 1
    rng = np.random.default_rng(7)
    (seg, S) = H.labelField(field, rng)
    colours = utils.writeRandomColourTable(None, S + 1, seed=5).columns
    rgba = np.stack([colours[k] for k in ('Red', 'Green', 'Blue', 'Alpha')], -1)
    blockPixels = 9 * H.NC
    assert (9 * H.NC) % 4 != 0
    (results, errors) = H.runRankThreads(world, _renderBody(seg, cuts, colours, S + 1, blockPixels))
    assert not any(errors), errors
    for (r, ((rows, packed), (rows2, packed2), sunk, info)) in enumerate(results):
        (lo, hi) = (cuts[r], cuts[r + 1])
        want = rgba[seg[lo:hi]]
        assert rows.dtype == np.uint8 and rows.shape == (hi - lo, H.NC, 4) and np.array_equal(rows, want), r
        assert rows2 is None and packed2 is None
        assert [(a, b) for (a, b, _v) in sunk] == [(y, min(y + 9 * distributed.RENDER_GROUP_BLOCKS, hi - lo))
                                                   for y in range(0, hi - lo, 9 * distributed.RENDER_GROUP_BLOCKS)], r
        if hi > lo:
            assert np.array_equal(np.concatenate([v for (_a, _b, v) in sunk]), want), r
        assert info['blocks'] == (hi - lo + 8) // 9
        (rects, npacked) = _rects(hi - lo)
        if npacked == 0:
            assert packed is None
            continue
        flat = seg[lo:hi].ravel()
        for (src0, rs, cs, nr, nc, dst0) in rects.tolist():
            idx = src0 + np.arange(nr)[:, None] * rs + np.arange(nc)[None, :] * cs
            assert np.array_equal(packed[dst0:dst0 + nr * nc].reshape(nr, nc, 4), rgba[flat[idx]]), r


@pytest.mark.parametrize('rowsOf', [pytest.param(lambda top: top, id='one-row-short'),
                                    pytest.param(lambda top: 300, id='300-rows')])
def test_label_without_a_row_raises_on_every_rank(rowsOf):
    """a table one row too short for the labels of field 'B', and one of 300 rows (the labels grow down the image,
    so the ranks miss different ones): every rank raises, naming the smallest missing label of ALL ranks, and
    returns"""
    from pyshepseg_amd import utils
    cuts = [0, 70, 140, 203]
    rng = np.random.default_rng(7)
    (seg, S) = H.labelField('B', rng)
    top = int(seg.max())
    nTable = rowsOf(top)
    missing = [int(v) for v in np.unique(seg) if v >= nTable]
    perRank = [sorted(int(v) for v in np.unique(seg[a:b]) if v >= nTable) for (a, b) in zip(cuts, cuts[1:])]
    if nTable == top:
        assert missing == [top] and sum(1 for m in perRank if m) >= 1
    else:
        firsts = [m[0] for m in perRank]                      # every rank misses labels, each another smallest one
        assert len(set(firsts)) == 3 and min(firsts) == missing[0]
    colours = utils.writeRandomColourTable(None, S + 1, seed=5).columns
    (results, errors) = H.runRankThreads(3, _renderBody(seg, cuts, colours, nTable, 9 * H.NC), timeout=120)
    assert results == [None] * 3
    for (r, e) in enumerate(errors):
        assert isinstance(e, utils.PyShepSegUtilsError), (r, e)
        assert 'segment id %d is not in the colour table (%d rows)' % (missing[0], nTable) in str(e), (r, e)


# ------------------------------------------------------------------------------------------
# 4. through the driver
# ------------------------------------------------------------------------------------------
def _checkDriverRun(world, tmp_path, tag):
    import dist_worker_colour_gpu as W
    base = str(tmp_path / tag)
    parts = [np.load('%s_rank%d.npz' % (base, r)) for r in range(world)]
    mosaic = np.load(base + '_labels.npy')
    S = int(parts[0]['maxSegId'])
    assert int(mosaic.max()) == S
    # numpy's table from the mean columns of the run
    want = {}
    stretch = []
    for (name, colour) in zip(W.NAMES, ('Red', 'Green', 'Blue')):
        col = parts[0][name]
        assert col.dtype == np.float32 and col.shape == (S + 1,)
        (want[colour], lohi) = _numpyStretch(col)
        stretch.append(lohi)
    want['Alpha'] = np.full(S + 1, 255, dtype=np.uint8)
    for (r, q) in enumerate(parts):                           # the same table on every rank
        for k in ('Red', 'Green', 'Blue', 'Alpha'):
            assert q[k].dtype == np.uint8 and np.array_equal(q[k], want[k]), (tag, r, k)
        assert np.array_equal(q['stretch'].view(np.uint64), np.array(stretch, dtype=np.float64).view(np.uint64)), (tag, r)
        assert int(q['onEngine']) == 1 and int(q['freed']) == 1 and int(q['returned']) == 1
        for name in W.NAMES:
            assert np.array_equal(q[name].view(np.uint32), parts[0][name].view(np.uint32))
        from pyshepseg_amd import distributed
        assert tuple(q['rows']) == distributed.colourShares(S + 1, world)[r]
        assert int(q['exchange_bytes']) == (3 * ((8 * 512 + 1) * 8 * world + S + 1) if world > 1 else 0)
        if int(q['outHi']) > int(q['outLo']):
            assert int(q['blocks']) == (int(q['outHi']) - int(q['outLo']) + 59) // 60 and int(q['blocks']) > 4
    rgba = np.stack([want[k] for k in ('Red', 'Green', 'Blue', 'Alpha')], -1)
    got = np.load(base + '_rgba.npy')
    assert got.dtype == np.uint8 and got.shape == (1500, 1300, 4)
    assert np.array_equal(got, rgba[mosaic]), tag
    for lvl in W.LEVELS:
        layer = np.load('%s_labels_ov%d.npy' % (base, lvl))
        ov = np.load('%s_rgba_ov%d.npy' % (base, lvl))
        assert ov.shape == ((1500 + lvl - 1) // lvl, (1300 + lvl - 1) // lvl, 4) and ov.dtype == np.uint8
        assert np.array_equal(ov, rgba[layer]), (tag, lvl)
    return got, parts


def _runDriver(world, transport, tag, tmp_path, env=None, ranges=None):
    dist_cases.runRanks(world, [os.path.join(ROOT, 'tests', 'dist_worker_colour_gpu.py'), str(tmp_path), transport, tag] +
                        ([dist_cases.encodeRanges(ranges)] if ranges else []), tmp_path, 900, extra_env=env)


def test_through_the_driver_two_socket_ranks(tmp_path):
    """the 1500 x 1300 synthetic raster from segmentation to rgba.npy over two socket ranks that share GPU 0 (device
    buffers staged through the host): the picture == numpy's lookup of the assembled mosaic through numpy's table,
    every overview layer == the lookup of the label layer of the same run; and the same picture when the ranks
    share output rows (SHEPSEG_SHARD=tiles, sequential stitch, a rank boundary in the middle of a tile row)"""
    _runDriver(2, 'socket', 'rows', tmp_path, env={'SHEPSEG_SHARD': 'rows'})
    (rows, parts) = _checkDriverRun(2, tmp_path, 'rows')
    assert sorted(tuple(int(v) for v in (q['outLo'], q['outHi'])) for q in parts)[0][1] <= \
        sorted(tuple(int(v) for v in (q['outLo'], q['outHi'])) for q in parts)[1][0]
    # (2 x 3 tiles: three tiles per rank cut the middle tile row, which the driver's own sharding of this grid does not)
    _runDriver(2, 'socket', 'tiles', tmp_path, env={'SHEPSEG_SHARD': 'tiles', 'SHEPSEG_STITCH': 'sequential'},
               ranges=[(0, 3), (3, 6)])
    (tiles, parts) = _checkDriverRun(2, tmp_path, 'tiles')
    assert [tuple(int(v) for v in q['tiles']) for q in parts] == [(0, 3), (3, 6)]
    spans = sorted((int(q['outLo']), int(q['outHi'])) for q in parts)
    assert spans[0][1] > spans[1][0]                          # the ranks share output rows
    assert np.array_equal(tiles, rows)


def test_through_the_driver_rccl_world_one(tmp_path):
    """the same pipeline with an RcclComm at world size 1 (the communicator on the device)"""
    _runDriver(1, 'rccl', 'rccl', tmp_path)
    _checkDriverRun(1, tmp_path, 'rccl')


# ------------------------------------------------------------------------------------------
# 5. from files at world 1
# ------------------------------------------------------------------------------------------
def test_from_files_world_one(tmp_path, oracle):
    """doTiledShepherdSegmentationDistributed(keepOutput=True), then the two new calls: the file ==
    utils.renderColourTable of the written label file through the one-GPU table of the same columns; a random table
    passed in paints the rows this rank holds"""
    from pyshepseg_amd import distributed, tiling, utils
    img = oracle.synthimg(11, 6, 1500, 1300)
    np.save(tmp_path / 'img.npy', img)
    entries = [(1, [('m1', 'mean')]), (2, [('m2', 'mean'), ('n2', 'pixcount')]), (3, [('med3', 'median')])]
    cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=3)
    res = distributed.doTiledShepherdSegmentationDistributed(
        str(tmp_path / 'img.npy'), str(tmp_path / 'out.npy'), tileSize=512, overlapSize=128, minSegmentSize=50,
        numClusters=30, fixedKMeansInit=True, bandNumbers=[2, 4, 5], concurrencyCfg=cfg, keepOutput=True)
    try:
        comm = res.engine.comm
        (ic, fc, fast) = distributed.calcPerSegmentStatsDistributedBands(res.engine, comm, res.hist, entries)
        columns = distributed.statsColumnsByName(entries, ic, fc, fast)
        table = distributed.writeColorTableFromRatColumnsDistributed(res.engine, comm, columns, 'm1', 'med3', 'm2')
        assert distributed.renderColourTableDistributed(res.engine, comm, res.dist, outfile=str(tmp_path / 'rgba.npy')) is None
        rnd = utils.writeRandomColourTable(None, res.maxSegId + 1, seed=3)
        (rows, span) = distributed.renderColourTableDistributed(res.engine, comm, res.dist, colours=rnd)
        with pytest.raises(utils.PyShepSegUtilsError, match='segment id %d is not in the colour table' % res.maxSegId):
            distributed.renderColourTableDistributed(
                res.engine, comm, res.dist, colours={k: v[:-1] for (k, v) in rnd.columns.items()})
    finally:
        res.engine.release()
    assert res.engine.colourTable is None
    one = utils.writeColorTableFromRatColumns(columns, 'm1', 'med3', 'm2')
    for k in ('Red', 'Green', 'Blue', 'Alpha'):
        assert np.array_equal(table.columns[k], one.columns[k]), k
    assert np.array_equal(np.array(table.stretch).view(np.uint64), np.array(one.stretch).view(np.uint64))
    assert columns['med3'].dtype == np.int64 and columns['m1'].dtype == np.float32
    utils.renderColourTable(str(tmp_path / 'out.npy'), one, outfile=str(tmp_path / 'want.npy'))
    assert np.array_equal(np.load(tmp_path / 'rgba.npy'), np.load(tmp_path / 'want.npy'))
    labels = np.load(tmp_path / 'out.npy')
    for lvl in tiling.overviewLevels(1300, 1500):
        rgba = np.stack([one.columns[k] for k in ('Red', 'Green', 'Blue', 'Alpha')], -1)
        assert np.array_equal(np.load(tmp_path / ('rgba_ov%d.npy' % lvl)), rgba[np.load(tmp_path / ('out_ov%d.npy' % lvl))])
    assert span == (0, 1500)
    assert np.array_equal(rows, np.stack([rnd.columns[k] for k in ('Red', 'Green', 'Blue', 'Alpha')], -1)[labels])
