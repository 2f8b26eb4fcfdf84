"""CPU: the multi-rank driver's file output (distributed.writeOutputDistributed, overviewPlan, readSlice and the
argument errors of doTiledShepherdSegmentationDistributed), with the oracle engine over the socket transport."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT

import dist_cases
from dist_output_helpers import simulateOverview

LEVELS = [2 ** k for k in range(1, 11)]


def _randomGrid(rng):
    (nr, nc) = (int(rng.integers(1, 401)), int(rng.integers(1, 401)))
    tile = int(rng.integers(2, 161))
    ov = 2 * int(rng.integers(0, (tile - 1) // 2 + 1))
    return nr, nc, tile, ov


def _checkPlan(nr, nc, tile, ov, lvl, what):
    """the owned rectangles of every tile against the chain-order writes of the one-GPU driver"""
    from pyshepseg_amd import distributed
    ti = dist_cases.tileInfoOf(nr, nc, tile, ov)
    mosaic = np.zeros((nr, nc), dtype=np.uint32)
    (_layer, owner) = simulateOverview(mosaic, ti, ov, lvl)
    tiles = [(c, r) for r in range(ti.nrows) for c in range(ti.ncols)]
    plan = distributed.overviewPlan(ti, ov, lvl, tiles)
    got = np.full(owner.shape, -1, dtype=np.int64)
    for (t, p) in enumerate(plan):
        if p is None:
            continue
        (x0, y0, x1, y1, sx, sy) = p
        assert 0 <= x0 < x1 <= owner.shape[1] and 0 <= y0 < y1 <= owner.shape[0], (what, t, p)
        assert (got[y0:y1, x0:x1] == -1).all(), ('rectangles overlap', what, t)          # disjoint
        got[y0:y1, x0:x1] = t
        (col, row) = tiles[t]
        (xpos, ypos, _xs, _ys) = ti.getTile(col, row)
        assert sx >= xpos and sy >= ypos, (what, t)
    # union == the written pixels, and every pixel belongs to the last tile that writes it
    assert np.array_equal(got, owner), (what, np.argwhere(got != owner)[:5])
    # a rank's rectangles come from its own tiles: the plan of any subset is the whole plan's restriction
    nt = len(tiles)
    for (t0, t1) in [(0, nt // 3), (nt // 3, nt // 2), (nt // 2, nt)]:
        sub = distributed.overviewPlan(ti, ov, lvl, tiles[t0:t1])
        assert sub == plan[t0:t1], what


def test_overview_plan_matches_chain_order_writes():
    """Random grids (rasters 1..400 px a side, tile and overlap as getTilesForFile allows, levels 2..1024) and
    the 300 x 260 / tile 100 / overlap 20 grid, whose tile rows 0 and 1 share overview rows at levels 16 and 32
    and leave holes: the plan's rectangles are disjoint, cover exactly the pixels the one-GPU driver writes,
    each pixel going to the last tile (row-major) that writes it."""
    rng = np.random.default_rng(20261016)
    n = 0
    overlaps = holes = 0
    for case in range(300):
        (nr, nc, tile, ov) = _randomGrid(rng)
        for lvl in rng.choice(LEVELS, size=2, replace=False):
            _checkPlan(nr, nc, tile, ov, int(lvl), (case, nr, nc, tile, ov, int(lvl)))
            n += 1
    for lvl in (2, 4, 8, 16, 32, 64):
        _checkPlan(300, 260, 100, 20, lvl, ('300x260', lvl))
    # the named grid has both overlapping blocks and holes at levels 16 and 32
    ti = dist_cases.tileInfoOf(300, 260, 100, 20)
    for lvl in (16, 32):
        (_l, owner) = simulateOverview(np.zeros((300, 260), np.uint32), ti, 20, lvl)
        holes += int((owner < 0).sum())
        from pyshepseg_amd import distributed
        b0 = distributed._overviewBlock(ti, 20, lvl, 0, 0, owner.shape[1], owner.shape[0])
        b1 = distributed._overviewBlock(ti, 20, lvl, 0, 1, owner.shape[1], owner.shape[0])
        overlaps += int(b1 is not None and b0 is not None and b1[1] < b0[3])
    assert n == 600 and holes > 0 and overlaps == 2


class _Recording(object):
    """a source that records which rows are read"""
    def __init__(self, arr):
        from pyshepseg_amd import tiling
        self.inner = tiling._ArraySource(arr)
        (self.shape, self.dtype) = (arr.shape, arr.dtype)
        self.RasterXSize, self.RasterYSize = arr.shape[2], arr.shape[1]
        self.rows = []

    def readRowsInto(self, bands, y0, y1, out):
        self.rows.append((list(bands), y0, y1))
        self.inner.readRowsInto(bands, y0, y1, out)

    def read(self, *a):
        raise AssertionError('readSlice reads whole rows only')


@pytest.mark.parametrize('kind', ['npy_u16', 'u8', 'i8', 'i64_pos', 'i64_neg'])
def test_read_slice_rows_and_types(kind, tmp_path):
    """readSlice returns exactly the selected bands of rows [yLo, yHi), in the pixel type the one-GPU path
    segments (as _lib.as_image converts), and reads no other rows"""
    from pyshepseg_amd import _lib, distributed, tiling
    rng = np.random.default_rng(3)
    arr = rng.integers(0, 250, size=(4, 53, 31))
    if kind == 'npy_u16':
        np.save(tmp_path / 'in.npy', arr.astype(np.uint16))
        src = tiling._open_source(str(tmp_path / 'in.npy'))
        assert isinstance(src.arr, np.memmap)
    else:
        dt = {'u8': np.uint8, 'i8': np.int8, 'i64_pos': np.int64, 'i64_neg': np.int64}[kind]
        a = arr.astype(dt)
        if kind == 'i8':
            a = (arr - 120).astype(np.int8)
        if kind == 'i64_neg':
            a = a - 100
        src = tiling._open_source(a)
    want_dtype = {'npy_u16': np.uint16, 'u8': np.uint8, 'i8': np.int16, 'i64_pos': np.uint32,
                  'i64_neg': np.int32}[kind]
    rec = _Recording(src.arr)
    for (bands, y0, y1) in [([3, 1], 7, 20), ([1, 2, 3, 4], 0, 53), ([2], 52, 53), ([4], 10, 10)]:
        rec.rows = []
        got = distributed.readSlice(rec, bands, y0, y1)
        want = _lib.as_image(np.ascontiguousarray(src.arr[[b - 1 for b in bands], y0:y1]))[0] if y1 > y0 else None
        assert got.dtype == np.dtype(want_dtype) or y1 == y0
        assert got.shape == (len(bands), y1 - y0, 31) and got.flags['C_CONTIGUOUS']
        if want is not None:
            assert np.array_equal(got, want) and got.dtype == want.dtype
            assert rec.rows == [([b - 1 for b in bands], y0, y1)]
    with pytest.raises(TypeError):
        distributed.readSlice(tiling._open_source(np.zeros((1, 4, 4), np.float32)), [1], 0, 4)
    with pytest.raises(TypeError):
        distributed.readSlice(tiling._open_source(np.full((1, 4, 4), 2 ** 40, np.int64)), [1], 0, 4)


def _run(world, what, jobs, tmp_path, timeout=600):
    with open(str(tmp_path / 'jobs.json'), 'w') as f:
        json.dump(jobs, f)
    dist_cases.runRanks(world, [os.path.join(ROOT, 'tests', 'dist_worker_output.py'), str(tmp_path), what,
                                str(tmp_path / 'jobs.json')], tmp_path, timeout, extra_env={'OMP_NUM_THREADS': '1'})


def _midRowRanges(ncols, nt, world):
    return [rs for rs in dist_cases.validRanges(ncols, nt, world) if dist_cases._midRowStart(rs, ncols)
            and all(b > a for (a, b) in rs)][0]


@pytest.mark.parametrize('world', [2, 3])
def test_output_stage_files_equal_one_process_oracle(world, tmp_path, oracle):
    """runDistributed + writeOutputDistributed with the oracle engine, sharded by rows, by tiles and by ranges
    whose boundaries fall in the middle of a tile row: the mosaic, the histogram and every overview layer file
    equal the one-process oracle mosaic, its histogram and the simulated chain-order overview writes"""
    from pyshepseg_amd import tiling
    levels = [2, 4, 8, 16, 32]
    jobs, refs = [], {}
    for seed in (0, 7):
        case = dist_cases.fuzzCase(seed, oracle)
        np.save(tmp_path / ('img%d.npy' % seed), case['img'])
        np.save(tmp_path / ('centres%d.npy' % seed), case['centres'])
        refs[seed] = (case, dist_cases.sequentialReference(case, oracle))
        common = dict(img=str(tmp_path / ('img%d.npy' % seed)), centres=str(tmp_path / ('centres%d.npy' % seed)),
                      msd=case['msd'], tile=case['tile'], ov=case['ov'], minseg=case['minseg'], null=case['null'],
                      four=case['four'], levels=levels)
        for (tag, ranges, env) in [
                ('rows', None, {'SHEPSEG_STITCH': 'parallel', 'SHEPSEG_SHARD': 'rows'}),
                ('tiles', None, {'SHEPSEG_STITCH': 'sequential', 'SHEPSEG_SHARD': 'tiles'}),
                ('midrow', _midRowRanges(case['ncols'], case['ntiles'], world), {'SHEPSEG_STITCH': 'parallel'})]:
            jobs.append(dict(common, ranges=ranges, env=env, out='s%d_%s' % (seed, tag)))
    _run(world, 'stage', jobs, tmp_path)
    midrowSeen = sharedRows = False
    for job in jobs:
        seed = int(job['out'][1:].split('_')[0])
        (case, (want, mx, hist)) = refs[seed]
        base = str(tmp_path / job['out'])
        assert np.array_equal(np.load(base + '.npy'), want), job['out']
        assert np.array_equal(np.load(base + '_hist.npy'), hist), job['out']
        ti = dist_cases.tileInfoOf(case['nr'], case['nc'], case['tile'], case['ov'])
        for lvl in levels:
            (layer, _owner) = simulateOverview(want, ti, case['ov'], lvl)
            assert np.array_equal(np.load(base + '_ov%d.npy' % lvl), layer), (job['out'], lvl)
        parts = [json.load(open('%s_rank%d.json' % (base, r))) for r in range(world)]
        stats = [list(kv) for kv in tiling.estimateStatsFromHisto(hist)]
        for q in parts:
            assert q['maxSegId'] == mx and q['stats'] == stats, job['out']
        if job['ranges']:
            assert [tuple(q['tiles']) for q in parts] == [tuple(r) for r in job['ranges']]
            midrowSeen = True
        rows = sorted(tuple(q['outRows']) for q in parts if q['outRows'][1] > q['outRows'][0])
        sharedRows = sharedRows or any(a[1] > b[0] for (a, b) in zip(rows, rows[1:]))
    assert midrowSeen and sharedRows        # (ranks that share output rows wrote windows, not rows)


def test_entry_point_argument_errors_on_every_rank(tmp_path):
    """doTiledShepherdSegmentationDistributed: a .kea outfile, an outfile in a directory that does not exist,
    an odd overlap, a band number out of range on one rank only and a floating-point raster each raise the
    same error (type and message) on every rank, nothing hangs, the .kea file is not created and the
    communicator passed in stays open"""
    img = np.zeros((3, 40, 30), dtype=np.uint16)
    np.save(tmp_path / 'img.npy', img)
    np.save(tmp_path / 'flt.npy', img.astype(np.float32))
    inf = str(tmp_path / 'img.npy')
    jobs = [
        dict(infile=inf, outfile=str(tmp_path / 'o.kea'), kw={}, rankKw=None, out='kea'),
        dict(infile=inf, outfile=str(tmp_path / 'missing' / 'o.npy'), kw={}, rankKw=None, out='nodir'),
        dict(infile=inf, outfile=str(tmp_path / 'o1.npy'), kw={'overlapSize': 5, 'tileSize': 20}, rankKw=None,
             out='odd'),
        dict(infile=inf, outfile=str(tmp_path / 'o2.npy'), kw={'bandNumbers': [1, 2]},
             rankKw={'1': {'bandNumbers': [1, 4]}}, out='bands'),
        dict(infile=str(tmp_path / 'flt.npy'), outfile=str(tmp_path / 'o3.npy'), kw={}, rankKw=None, out='float'),
    ]
    world = 3
    _run(world, 'errors', jobs, tmp_path, timeout=300)
    want = {'kea': ('PyShepSegTilingError', '.npy'), 'nodir': ('PyShepSegTilingError', 'writable directory'),
            'odd': ('PyShepSegTilingError', 'even'), 'bands': ('PyShepSegTilingError', 'out of range'),
            'float': ('TypeError', 'integer')}
    for job in jobs:
        got = [json.load(open(str(tmp_path / ('%s_rank%d.json' % (job['out'], r))))) for r in range(world)]
        assert all(g is not None for g in got), (job['out'], got)
        assert len({tuple(g) for g in got}) == 1, (job['out'], got)
        (typ, frag) = want[job['out']]
        assert got[0][0] == typ and frag in got[0][1], (job['out'], got[0])
    assert not os.path.exists(str(tmp_path / 'o.kea'))
    for n in ('o1.npy', 'o2.npy', 'o3.npy'):
        assert not os.path.exists(str(tmp_path / n))
