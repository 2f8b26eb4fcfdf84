"""GPU: distributed.doTiledShepherdSegmentationDistributed from a .npy raster to .npy files, every rank on GPU 0
(socket transport; RCCL at world size 1), against tiling.doTiledShepherdSegmentation of the same input in the
test process: every file equal (np.array_equal), and the result fields."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT

import dist_cases

pytestmark = pytest.mark.gpu

KW = dict(tileSize=512, overlapSize=128, minSegmentSize=50, numClusters=30, fixedKMeansInit=True,
          bandNumbers=[1, 3, 5])
LEVELS = [2, 4, 8, 16]


def _launch(world, transport, jobs, tmp_path, timeout=600):
    with open(str(tmp_path / 'jobs.json'), 'w') as f:
        json.dump(jobs, f)
    dist_cases.runRanks(world, [os.path.join(ROOT, 'tests', 'dist_worker_output_gpu.py'), str(tmp_path), transport,
                                str(tmp_path / 'jobs.json')], tmp_path, timeout)


def _oneGpu(infile, outfile, levels, monkeypatch, **kw):
    from pyshepseg_amd import tiling
    if levels is not None:
        monkeypatch.setattr(tiling, 'overviewLevels', lambda xs, ys: list(levels))
    cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=3)
    r = tiling.doTiledShepherdSegmentation(infile, outfile, concurrencyCfg=cfg, **kw)
    monkeypatch.undo()
    return r


def _files(levels):
    return ['', '_hist'] + ['_ov%d' % lvl for lvl in levels]


def _checkAgainst(ref, refBase, base, levels, world, what):
    for r in range(world):
        assert not os.path.exists('%s_rank%d.err' % (base, r)), (what, r, open('%s_rank%d.err' % (base, r)).read())
    for suffix in _files(levels):
        want = np.load(refBase + suffix + '.npy')
        got = np.load(base + suffix + '.npy')
        assert got.dtype == want.dtype and np.array_equal(got, want), (what, suffix)
    parts = [np.load('%s_rank%d.npz' % (base, r)) for r in range(world)]
    for q in parts:
        assert int(q['maxSegId']) == ref.maxSegId and np.array_equal(q['hist'], ref.hist), what
        assert np.array_equal(q['centres'], ref.kmeans.cluster_centers_), what
        assert float(q['msd']) == float(ref.maxSpectralDiff), what
        assert float(q['subsamplePcnt']) == (-1.0 if ref.subsamplePcnt is None else float(ref.subsamplePcnt)), what
        assert (int(q['numTileRows']), int(q['numTileCols'])) == (ref.numTileRows, ref.numTileCols), what
        assert bool(q['hasEmpty']) == bool(ref.hasEmptySegments), what
        assert q['stats'].tolist() == ['%s=%s' % kv for kv in ref.bandStatistics], what
        assert int(q['noSeg']) == 1
        assert {'walltime', 'reading', 'writing'} <= set(json.loads(str(q['timings']))), what
    return parts


@pytest.fixture(scope='module')
def synth(tmp_path_factory):
    from oracle import oracle
    d = tmp_path_factory.mktemp('synth')
    np.save(d / 'img.npy', oracle.synthimg(11, 6, 1500, 1300))
    return d


@pytest.fixture(scope='module')
def synthRef(synth):
    mp = pytest.MonkeyPatch()
    ref = _oneGpu(str(synth / 'img.npy'), str(synth / 'ref.npy'), LEVELS, mp, **KW)
    return ref, str(synth / 'ref')


# (world, transport, [(tag, stitch form, shard form, ranges)])
RUNS = [
    pytest.param(1, 'env', [('seq', 'sequential', None, None), ('par', 'parallel', None, None)], id='world1'),
    pytest.param(2, 'socket', [('par_rows', 'parallel', 'rows', None), ('seq_tiles', 'sequential', 'tiles', None)],
                 id='world2'),
    pytest.param(3, 'socket', [('midrow', 'parallel', None, [(0, 3), (3, 5), (5, 6)]),
                               ('seq_tiles', 'sequential', 'tiles', None)], id='world3-midrow'),
    pytest.param(4, 'socket', [('par', 'parallel', 'rows', None), ('seq_tiles', 'sequential', 'tiles', None)],
                 id='world4'),
]


@pytest.mark.parametrize('world,transport,forms', RUNS)
def test_distributed_files_equal_one_gpu(world, transport, forms, synth, synthRef, tmp_path):
    """the 6-band 1500 x 1300 raster (tile 512, overlap 128, k = 30, bands 1, 3, 5) at world sizes 1-4, both
    stitch forms, both shard forms and a rank boundary in the middle of a tile row"""
    (ref, refBase) = synthRef
    jobs = []
    for (tag, stitch, shard, ranges) in forms:
        env = {'SHEPSEG_STITCH': stitch}
        if shard:
            env['SHEPSEG_SHARD'] = shard
        jobs.append(dict(infile=str(synth / 'img.npy'), outfile=str(tmp_path / (tag + '.npy')), kw=KW, env=env,
                         levels=LEVELS, ranges=ranges, stats=None, out=tag))
    _launch(world, transport, jobs, tmp_path)
    for (tag, stitch, _shard, ranges) in forms:
        parts = _checkAgainst(ref, refBase, str(tmp_path / tag), LEVELS, world, tag)
        assert {str(q['mode']).split('->')[0] for q in parts} == {stitch}, tag
        if ranges:
            assert [tuple(int(v) for v in q['tiles']) for q in parts] == [tuple(r) for r in ranges]


def test_keep_output_statistics_world2(synth, synthRef, tmp_path):
    """keepOutput=True: calcPerSegmentStatsDistributed on result.engine (imgbandnum 2 = band 3, the second of
    bandNumbers) equals tilingstats.calcPerSegmentStats of the one-GPU mosaic, bit for bit"""
    from pyshepseg_amd import tilingstats
    from oracle import oracle
    (ref, refBase) = synthRef
    _launch(2, 'socket', [dict(infile=str(synth / 'img.npy'), outfile=str(tmp_path / 'k.npy'), kw=KW,
                               env={'SHEPSEG_SHARD': 'rows'}, levels=LEVELS, ranges=None, stats=2, out='k')],
            tmp_path)
    parts = _checkAgainst(ref, refBase, str(tmp_path / 'k'), LEVELS, 2, 'keep')
    band = oracle.synthimg(11, 6, 1500, 1300)[2]
    from dist_worker_output_gpu import SEL
    wic, wfc, _f = tilingstats.calcPerSegmentStats(np.load(refBase + '.npy'), band, SEL, maxSegId=ref.maxSegId)
    for q in parts:
        assert np.array_equal(q['ic'], wic)
        assert np.array_equal(q['fc'].view(np.uint32), wfc.view(np.uint32))


def test_rccl_world1(synth, synthRef, tmp_path):
    """the entry point with an explicit RcclComm (world size 1)"""
    (ref, refBase) = synthRef
    _launch(1, 'rccl', [dict(infile=str(synth / 'img.npy'), outfile=str(tmp_path / 'r.npy'), kw=KW, env={},
                             levels=LEVELS, ranges=None, stats=None, out='r')], tmp_path)
    _checkAgainst(ref, refBase, str(tmp_path / 'r'), LEVELS, 1, 'rccl')


def test_reference_overview_goldens(golden, tmp_path):
    """the reference's stitch fixtures at world 2 with levels [2, 4, 8] patched in the rank processes: mosaic ==
    the fixture's, every layer == the reference's overview golden, band statistics == its _stats entry"""
    gov = golden('overviews_stats')
    names = ['stitch_2x2', 'stitch_3x3_null', 'stitch_3x4_8conn']
    jobs = []
    for name in names:
        g = golden(name)
        np.save(tmp_path / (name + '_img.npy'), g['img'])
        np.save(tmp_path / (name + '_c.npy'), g['centres'])
        kw = dict(tileSize=int(g['tile_size']), overlapSize=int(g['overlap']), minSegmentSize=int(g['min_seg']),
                  maxSpectralDiff=float(g['msd']), imgNullVal=int(g['null_val']) if int(g['has_null']) else None,
                  fourConnected=bool(g['four']), centres=str(tmp_path / (name + '_c.npy')))
        jobs.append(dict(infile=str(tmp_path / (name + '_img.npy')), outfile=str(tmp_path / (name + '.npy')), kw=kw,
                         env={'SHEPSEG_SHARD': 'tiles', 'SHEPSEG_STITCH': 'sequential'}, levels=[2, 4, 8],
                         ranges=None, stats=None, out=name))
    _launch(2, 'socket', jobs, tmp_path)
    for name in names:
        g = golden(name)
        assert np.array_equal(np.load(tmp_path / (name + '.npy')), g['mosaic']), name
        for lvl in (2, 4, 8):
            assert np.array_equal(np.load(tmp_path / ('%s_ov%d.npy' % (name, lvl))), gov['%s_ov%d' % (name, lvl)])
        for r in range(2):
            q = np.load(tmp_path / ('%s_rank%d.npz' % (name, r)))
            assert q['stats'].tolist() == gov[name + '_stats'].tolist(), name


@pytest.mark.parametrize('world', [3, 4])
def test_overlapping_blocks_holes_and_empty_rank(world, tmp_path, monkeypatch):
    """300 x 260, tile 100, overlap 20, levels [2, 4, 16, 32]: at levels 16 and 32 the blocks of tile rows 0 and
    1 overlap and some layer pixels are covered by no block; world 3 = one tile row per rank, world 4 = one rank
    without tiles"""
    from oracle import oracle
    np.save(tmp_path / 'img.npy', oracle.synthimg(5, 3, 300, 260))
    kw = dict(tileSize=100, overlapSize=20, minSegmentSize=10, numClusters=10, fixedKMeansInit=True)
    levels = [2, 4, 16, 32]
    ref = _oneGpu(str(tmp_path / 'img.npy'), str(tmp_path / 'ref.npy'), levels, monkeypatch, **kw)
    _launch(world, 'socket', [dict(infile=str(tmp_path / 'img.npy'), outfile=str(tmp_path / 'o.npy'), kw=kw,
                                   env={'SHEPSEG_SHARD': 'rows'}, levels=levels, ranges=None, stats=None, out='o')],
            tmp_path)
    parts = _checkAgainst(ref, str(tmp_path / 'ref'), str(tmp_path / 'o'), levels, world, 'grid')
    ranges = [tuple(int(v) for v in q['tiles']) for q in parts]
    if world == 3:
        assert ranges == [(0, 2), (2, 4), (4, 6)]
    else:
        assert sum(1 for (a, b) in ranges if b == a) == 1


def test_errors_on_every_rank(tmp_path):
    """a .kea outfile, an outfile in a missing directory and an int64 raster whose rows on the last rank leave
    the 32-bit range (found while reading that rank's slice, inside runDistributed): every rank raises the
    same error, none hangs, and the .kea file is not created"""
    img = np.zeros((3, 300, 260), dtype=np.int64)
    img[:, 250:, :] = 2 ** 40
    np.save(tmp_path / 'big.npy', img)
    np.save(tmp_path / 'u16.npy', img.astype(np.uint16))
    kw = dict(tileSize=100, overlapSize=20, numClusters=4, fixedKMeansInit=True)
    jobs = [dict(infile=str(tmp_path / 'u16.npy'), outfile=str(tmp_path / 'o.kea'), kw=kw, out='kea'),
            dict(infile=str(tmp_path / 'u16.npy'), outfile=str(tmp_path / 'no' / 'o.npy'), kw=kw, out='nodir'),
            dict(infile=str(tmp_path / 'big.npy'), outfile=str(tmp_path / 'o.npy'), kw=kw, out='range',
                 env={'SHEPSEG_SHARD': 'rows'})]
    world = 2
    _launch(world, 'socket', jobs, tmp_path, timeout=300)
    want = {'kea': 'PyShepSegTilingError', 'nodir': 'PyShepSegTilingError', 'range': 'TypeError'}
    for job in jobs:
        got = []
        for r in range(world):
            p = tmp_path / ('%s_rank%d.err' % (job['out'], r))
            assert p.exists(), (job['out'], r)
            got.append(tuple(json.load(open(str(p)))))
        assert len(set(got)) == 1 and got[0][0] == want[job['out']], (job['out'], got)
    assert not (tmp_path / 'o.kea').exists()
