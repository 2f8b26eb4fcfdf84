"""CPU (socket transport, world_size 2 and 3): the multi-GPU driver's sharding, k-means gather/broadcast,
stitch chain with boundary exchange and histogram all-reduce, run with the oracle engine, must
reproduce the single-process tiled result exactly."""
import functools
import json
import os
import socket
import sys

import numpy as np
import pytest

from conftest import ROOT

import dist_cases


class _Ds(object):
    def __init__(self, ys, xs):
        self.RasterYSize, self.RasterXSize = ys, xs


def test_socket_comm_collectives(tmp_path):
    """the socket transport's point-to-point and collectives at world size 3"""
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from pyshepseg_amd import comm as C\n"
        "c = C.SocketComm()\n"
        "r, w = c.rank, c.world\n"
        "assert c.allgather_obj({'r': r}) == [{'r': i} for i in range(w)]\n"
        "assert c.bcast_obj('x' * 100000 if r == 1 else None, src=1) == 'x' * 100000\n"
        "assert c.allreduce_sum_i64(np.arange(5) * (r + 1)).tolist() == (np.arange(5) * sum(range(1, w + 1))).tolist()\n"
        "assert c.max_f64(1.5 * r) == 1.5 * (w - 1)\n"
        "a = np.arange(300000, dtype=np.uint32) + r\n"
        "c.send_bytes(a, (r + 1) %% w)\n"
        "b = np.frombuffer(c.recv_bytes((r - 1) %% w), dtype=np.uint32)\n"
        "assert np.array_equal(b, np.arange(300000, dtype=np.uint32) + (r - 1) %% w)\n"
        "c.barrier(); c.close()\n" % ROOT)
    _run_ranks(3, ['-c', code], tmp_path, timeout=120)


def test_shard_tile_rows():
    from pyshepseg_amd import tiling, distributed
    ti = tiling.getTilesForFile(_Ds(40000, 40000), 4096, 1024)
    for world in (1, 2, 3, 4, 8, 12, 16):
        sh = distributed.shardTileRows(ti, world)
        assert len(sh) == world
        rows = [r for (a, b) in sh for r in range(a, b)]
        assert rows == list(range(ti.nrows))                       # contiguous, complete, ordered
        assert sum(1 for (a, b) in sh if b > a) == min(world, ti.nrows)
    sh = distributed.shardTileRows(ti, 8)
    assert max(b - a for (a, b) in sh) <= 2


def test_shard_tiles():
    from pyshepseg_amd import tiling, distributed
    ti = tiling.getTilesForFile(_Ds(40000, 40000), 4096, 1024)
    nt = ti.ncols * ti.nrows
    for world in (1, 2, 3, 4, 5, 8, 12, 16, 200):
        sh = distributed.shardTiles(ti, world)
        assert len(sh) == world
        assert [t for (a, b) in sh for t in range(a, b)] == list(range(nt))       # contiguous, complete
        ne = [(a, b) for (a, b) in sh if b > a]
        assert all(b - a >= ti.ncols for (a, b) in ne[:-1])         # top neighbours: local or previous rank
        for p, (a, b) in enumerate(sh):
            if b > a:
                for (kind, col, row, h, w) in distributed.boundaryPlan(ti, sh, p, 1024):
                    assert a <= row * ti.ncols + col < b
    sh = distributed.shardTiles(ti, 8)                               # 144 tiles, balanced by pixel area
    area = [sum(ti.getTile(t % 12, t // 12)[2] * ti.getTile(t % 12, t // 12)[3] for t in range(a, b))
            for (a, b) in sh]
    assert max(area) < 1.06 * min(area)
    assert [b - a for (a, b) in distributed.shardTiles(ti, 16)].count(12) == 12     # whole rows


def test_shard_plan_random_grids():
    """Random rasters / tile sizes / world sizes: every tile's top and left neighbours are either
    in the same shard or delivered by the previous shard's boundary plan."""
    from pyshepseg_amd import tiling, distributed
    rng = np.random.RandomState(7)
    for _case in range(200):
        (nr, nc) = (int(rng.randint(50, 3000)), int(rng.randint(50, 3000)))
        tile = int(rng.randint(32, 700))
        ov = 2 * int(rng.randint(1, max(2, tile // 4)))
        ti = tiling.getTilesForFile(_Ds(nr, nc), tile, ov)
        world = int(rng.randint(1, 12))
        sh = distributed.shardTiles(ti, world)
        nt = ti.ncols * ti.nrows
        assert [t for (a, b) in sh for t in range(a, b)] == list(range(nt))
        dist_cases.checkShardRanges(sh, ti.ncols, nt)
        dist_cases.checkNeighboursDelivered(ti, sh, ov)


def test_shard_range_checks_reject_bad_lists():
    """the checks the tests' own range lists go through: they must refuse what shardTiles never makes"""
    ti = dist_cases.tileInfoOf(252, 207, 56, 16)                    # 4 x 5 tiles
    (ncols, nt) = (ti.ncols, ti.ncols * ti.nrows)
    assert (ncols, nt) == (4, 20)
    for ok in ([(0, 11), (11, 20)], [(0, 4), (4, 4), (4, 20)], [(0, 20), (20, 20)], [(0, 0), (0, 7), (7, 20)]):
        dist_cases.checkShardRanges(ok, ncols, nt)
        dist_cases.checkNeighboursDelivered(ti, ok, 16)
    for bad in ([(0, 11), (12, 20)], [(0, 11), (11, 19)], [(11, 20), (0, 11)], [(0, 3), (3, 20)],
                [(0, 8), (8, 10), (10, 20)], [(0, 12), (12, 11), (11, 20)]):
        assert dist_cases.shardProblems(bad, ncols, nt), bad
    # a rank with fewer than ncols tiles before another: a top neighbour two ranks back goes undelivered
    with pytest.raises(AssertionError):
        dist_cases.checkNeighboursDelivered(ti, [(0, 8), (8, 10), (10, 20)], 16)
    # every list the enumeration yields passes both checks
    for w in (2, 3, 4):
        for rs in dist_cases.validRanges(ncols, nt, w):
            dist_cases.checkNeighboursDelivered(ti, rs, 16)


def _run_ranks(world, argv, tmp_path, timeout=600, extra_env=None):
    """start `world` rank processes with the environment a launcher sets; all must exit 0 (the first that
    does not, or a time-out, stops them all)"""
    env = {'OMP_NUM_THREADS': '1'}
    env.update(extra_env or {})
    return dist_cases.runRanks(world, argv, tmp_path, timeout, extra_env=env)


STITCH_GOLDEN = ['stitch_2x2', 'stitch_3x3_null', 'stitch_3x4_8conn', 'stitch_quirk_empties',
                 'stitch_quirk_zeros']


@pytest.mark.parametrize('name', STITCH_GOLDEN)
@pytest.mark.parametrize('world', [2, 3])
def test_parallel_stitch_equals_reference_mosaic(name, world, tmp_path):
    """The parallel (provisional-id) stitch of the sharded driver against the REFERENCE's own stitched
    mosaics, both quirk fixtures included: where a tile hands out an id that its trimmed window
    does not show (stitch_quirk_empties) the driver must notice and redo the stitch sequentially."""
    path = os.path.join(ROOT, 'tests', 'golden', name + '.npz')
    g = np.load(path, allow_pickle=True)
    _run_ranks(world, [os.path.join(ROOT, 'tests', 'dist_worker.py'), str(tmp_path), '0', '0', '0', path],
               tmp_path)
    parts = [np.load(tmp_path / ('rank%d.npz' % r)) for r in range(world)]
    want = g['mosaic']
    got = np.zeros_like(want)
    modes = set()
    for q in parts:
        lo, hi = int(q['outLo']), int(q['outHi'])
        got[lo:hi] = np.maximum(got[lo:hi], q['out'])
        assert int(q['maxSegId']) == int(g['max_seg_id'])
        assert np.array_equal(q['hist'], g['hist'])
        modes.add(str(q['mode']))
    assert np.array_equal(got, want)
    assert len(modes) == 1                       # every rank took the same decision
    redone = {int(q['redone']) for q in parts}
    ntiles = int(parts[0]['ntiles'])
    assert len(redone) == 1
    if name == 'stitch_quirk_empties':
        # the chain is redone only from the tile after the first one that hides an id it handed out: the
        # tiles up to it keep their (renumbered) result
        assert modes == {'parallel->sequential'}
        assert 0 < redone.pop() < ntiles
    elif name in ('stitch_2x2', 'stitch_3x3_null', 'stitch_3x4_8conn'):
        assert modes == {'parallel'} and redone == {0}


@pytest.mark.parametrize('world,simple,NR,mode,shard,order', [
    (2, 0, 330, 'parallel', 'rows', 'diagonal'), (3, 0, 330, 'parallel', 'tiles', 'diagonal'),
    (2, 1, 330, 'sequential', 'tiles', 'diagonal'), (3, 0, 150, 'parallel', 'rows', 'diagonal'),
    (3, 0, 330, 'sequential', 'tiles', 'diagonal'), (2, 0, 330, 'parallel', 'tiles', 'rowmajor'),
    (3, 0, 330, 'sequential', 'rows', 'diagonal'), (2, 0, 330, 'parallel', 'rows', 'rowmajor'),
    (2, 0, 330, 'parallel', 'tiles', 'diagonal')])
def test_two_rank_chain_matches_single_process(world, simple, NR, mode, shard, order, tmp_path, oracle):
    # order: a rank's chain steps of the parallel stitch along anti-diagonals or in row-major order
    # NR = 150: two tile rows for three ranks -> whole-row shards and a rank without tiles
    img = oracle.synthimg(31, 3, NR, 260)
    img[:, :4, :] = 65535                      # a null border row band (nulls are not given here)
    np.save(tmp_path / 'img.npy', img)
    tile, ov = 96, 32
    _run_ranks(world, [os.path.join(ROOT, 'tests', 'dist_worker.py'), str(tmp_path), str(tile), str(ov),
                       str(simple)], tmp_path,
               extra_env={'SHEPSEG_STITCH': mode, 'SHEPSEG_SHARD': shard, 'SHEPSEG_CHAIN_ORDER': order})
    parts = [np.load(tmp_path / ('rank%d.npz' % r)) for r in range(world)]
    assert {str(q['mode']).split('->')[0] for q in parts} == {mode}
    # single-process reference: oracle tiles + oracle stitch with the same centres
    centres, msd = parts[0]['centres'], float(parts[0]['msd'])
    for q in parts[1:]:
        assert np.array_equal(q['centres'], centres)
    tiles, ntc, ntr = oracle.get_tiles(NR, 260, tile, ov)
    local = {}
    for (c, r), (x, y, xs, ys) in tiles.items():
        sub = np.ascontiguousarray(img[:, y:y + ys, x:x + xs])
        local[(c, r)] = oracle.segment_tile(sub, centres, 12, msd, None, True)['segimg']
    want, mx, hist = oracle.stitch_tiles(local, tiles, ntc, ntr, NR, 260, ov, simple=bool(simple))
    got = np.zeros_like(want)
    cover = np.zeros(NR, dtype=bool)
    for q in parts:
        lo, hi = int(q['outLo']), int(q['outHi'])
        got[lo:hi] = np.maximum(got[lo:hi], q['out'])          # a rank writes only its tiles' windows
        cover[lo:hi] = True
        assert int(q['maxSegId']) == mx
        assert np.array_equal(q['hist'], hist)
    assert cover.all()
    assert np.array_equal(got, want)
    # per-segment statistics sharded the same way == the oracle on the whole raster, on every rank
    sel = [('a', 'min'), ('b', 'max'), ('c', 'mean'), ('d', 'stddev'), ('e', 'median'),
           ('f', 'mode'), ('g', 'percentile', 25), ('h', 'pixcount')]
    wic, wfc = oracle.segstats(want, np.ascontiguousarray(img[1]), sel, 65535, -9999, max_seg_id=mx)
    for r in range(world):
        st = np.load(tmp_path / ('stats%d.npz' % r))
        assert np.array_equal(st['ic'], wic)
        assert np.array_equal(st['fc'].view(np.uint32), wfc.view(np.uint32))
        # segments DO straddle the rank boundaries (their pixels travelled as raw arrays and were reduced by the
        # rank whose share of the id space holds them): the ids present in more than one rank's rows
        if world > 1:
            held = [set(np.unique(q['out'])) - {0} for q in parts]
            strad = set()
            for a in range(world):
                for b in range(a + 1, world):
                    strad |= held[a] & held[b]
            assert int(st['straddlers']) == len(strad) and (simple or NR < 330 or len(strad) > 0)


@pytest.mark.parametrize('seed', range(8))
def test_parallel_stitch_fuzz_in_process(seed, oracle):
    """One rank, both forms of the stitch on random small rasters with many tiles: identical mosaics,
    maxSegId and histograms whichever way the parallel form ends (kept, or redone sequentially)."""
    case = dist_cases.fuzzCase(seed, oracle)
    res = {}
    for mode in ('sequential', 'parallel'):
        out, r = dist_cases.runInProcess(case, oracle, mode)
        res[mode] = (out, r.maxSegId, r.hist.copy(), r.stitchMode)
    assert res['sequential'][3] == 'sequential'
    assert res['parallel'][3] in ('parallel', 'parallel->sequential')
    assert np.array_equal(res['sequential'][0], res['parallel'][0])
    assert res['sequential'][1] == res['parallel'][1]
    assert np.array_equal(res['sequential'][2], res['parallel'][2])


# ------------------------------------------------------------------------------------------
# the partial redo of the parallel stitch across rank boundaries
# ------------------------------------------------------------------------------------------
FUZZ_SEEDS = range(40)
WORKER = os.path.join(ROOT, 'tests', 'dist_worker.py')


@functools.lru_cache(maxsize=None)
def _fuzzCases():
    """The fuzz recipe's rasters with the one-rank parallel stitch's outcome ('mode1', 'redone1', and `bad`,
    None unless it ended in a partial redo) and the sequential stitch of the oracle tiles ('want')."""
    from oracle import oracle
    oracle.build()
    out = []
    for seed in FUZZ_SEEDS:
        case = dist_cases.fuzzCase(seed, oracle)
        _img, r = dist_cases.runInProcess(case, oracle, 'parallel')
        (case['mode1'], case['redone1']) = (r.stitchMode, r.chainStepsRedone)
        partial = r.stitchMode == 'parallel->sequential' and r.chainStepsRedone < case['ntiles']
        case['bad'] = case['ntiles'] - 1 - r.chainStepsRedone if partial else None
        case['want'] = dist_cases.sequentialReference(case, oracle)
        out.append(case)
    return tuple(out)


def _redoCases():
    return [c for c in _fuzzCases() if c['bad'] is not None]


@functools.lru_cache(maxsize=None)
def _placementPlan(world):
    """(case, placement, ranges): for every raster that ends in a partial redo, one valid range list per
    placement of `bad` that exists at this world size"""
    return tuple((case, name, ranges) for case in _redoCases()
                 for (name, ranges) in dist_cases.pickRanges(case['ncols'], case['ntiles'], world, case['bad']))


def _runJobs(world, jobs, tmp_path, timeout=300):
    """jobs: (case, ranges or None, environment, tag), all run by one launch of `world` ranks over one
    communicator; each checked against the sequential stitch.  Returns {tag: the ranks' results}."""
    fixtures, spec = {}, []
    for (case, ranges, env, tag) in jobs:
        if case['seed'] not in fixtures:
            fixtures[case['seed']] = str(tmp_path / ('seed%d.npz' % case['seed']))
            dist_cases.saveCase(case, fixtures[case['seed']])
        spec.append({'fixture': fixtures[case['seed']], 'ranges': ranges, 'env': env, 'out': tag})
    (tmp_path / 'jobs.json').write_text(json.dumps(spec))
    _run_ranks(world, [WORKER, str(tmp_path), 'cases', str(tmp_path / 'jobs.json')], tmp_path, timeout=timeout)
    res = {}
    for (case, ranges, env, tag) in jobs:
        res[tag] = [dict(np.load(tmp_path / ('%s_rank%d.npz' % (tag, r)))) for r in range(world)]
        dist_cases.checkRanksAgainst(case['want'], res[tag], tag)
    return res


@pytest.mark.parametrize('world', [2, 3, 4])
def test_partial_redo_at_every_boundary_placement(world, tmp_path):
    """Rasters whose parallel stitch ends in a partial redo (the chain redone sequentially from the tile
    after `bad`), with rank boundaries placed around `bad` on purpose: at the last tile of a rank that sends
    its strips on (also when the next rank starts mid-row, the 'r' strip), at a rank's first tile, inside a
    range, on the last rank; a rank all of whose tiles are redone, an empty rank between two others.  Both
    chain orders.  Every rank against the sequential stitch, and the redo must start where one rank says."""
    jobs = []
    for (case, name, ranges) in _placementPlan(world):
        dist_cases.checkShardRanges(ranges, case['ncols'], case['ntiles'])
        dist_cases.checkNeighboursDelivered(dist_cases.tileInfoOf(case['nr'], case['nc'], case['tile'], case['ov']),
                                            ranges, case['ov'])
        assert name in dist_cases.placementsOf(ranges, case['bad'], case['ncols'])
        for order in ('diagonal', 'rowmajor'):
            jobs.append((case, ranges, {'SHEPSEG_STITCH': 'parallel', 'SHEPSEG_CHAIN_ORDER': order},
                         'seed%d_%s_%s' % (case['seed'], name, order)))
    res = _runJobs(world, jobs, tmp_path)
    for (case, ranges, _env, tag) in jobs:
        parts = res[tag]
        assert [tuple(int(v) for v in q['tiles']) for q in parts] == [tuple(r) for r in ranges], tag
        for q in parts:
            assert str(q['mode']) == 'parallel->sequential', tag
            assert int(q['redone']) == case['ntiles'] - 1 - case['bad'], tag


def test_partial_redo_placements_all_exercised():
    """The placements above exist for the fuzz recipe's rasters: when a change of the recipe moves `bad`,
    this fails instead of the test above quietly checking something else."""
    assert len(_redoCases()) >= 5
    seen = {}
    for world in (2, 3, 4):
        for (case, _name, ranges) in _placementPlan(world):
            for p in dist_cases.placementsOf(ranges, case['bad'], case['ncols']):
                seen.setdefault(p, set()).add(world)
    assert set(seen) == set(dist_cases.PLACEMENTS), sorted(seen)
    for p in ('bad_last_of_sender', 'bad_last_of_sender_midrow', 'bad_first_of_rank', 'bad_mid_range',
              'bad_on_last_rank', 'rank_all_redone', 'midrow_boundary'):
        assert seen[p] == {2, 3, 4}, (p, seen[p])
    assert seen['empty_rank'] == {3, 4}


FUZZ_RUNS = [pytest.param(2, 'tiles', (7,), id='review-seed7-world2-tiles')] + [
    pytest.param(w, shard, None, id='world%d-%s' % (w, shard)) for w in (2, 3, 4) for shard in ('tiles', 'rows')]


@pytest.mark.parametrize('world,shard,seeds', FUZZ_RUNS)
def test_multi_rank_fuzz_matches_sequential(world, shard, seeds, tmp_path):
    """The fuzz recipe's rasters at world sizes 2-4 with the ranges shardTiles picks, both chain orders: every
    rank against the sequential stitch, and the stitch ends as the one-rank run does.  The first parameter is
    the case the partial redo once got wrong: seed 7, two ranks sharded by tiles, (0, 11) and (11, 20), with
    `bad` = 10 the last tile of rank 0 -- its strips went on to rank 1 with provisional ids."""
    from pyshepseg_amd import distributed
    cases = [c for c in _fuzzCases() if seeds is None or c['seed'] in seeds]
    jobs = [(c, None, {'SHEPSEG_STITCH': 'parallel', 'SHEPSEG_SHARD': shard, 'SHEPSEG_CHAIN_ORDER': order},
             'seed%d_%s' % (c['seed'], order)) for c in cases for order in ('diagonal', 'rowmajor')]
    res = _runJobs(world, jobs, tmp_path)
    for (case, _r, _env, tag) in jobs:
        parts = res[tag]
        ti = dist_cases.tileInfoOf(case['nr'], case['nc'], case['tile'], case['ov'])
        ranges = [tuple(int(v) for v in q['tiles']) for q in parts]
        assert ranges == distributed.shardTiles(ti, world, wholeRows=(shard == 'rows')), tag
        for q in parts:
            assert (str(q['mode']), int(q['redone'])) == (case['mode1'], case['redone1']), tag
    if seeds == (7,):
        (case,) = cases
        assert case['bad'] == 10 and ranges == [(0, 11), (11, 20)]
        assert 'bad_last_of_sender' in dist_cases.placementsOf(ranges, case['bad'], case['ncols'])


def test_socket_comm_handshake_and_private_rendezvous(tmp_path, monkeypatch):
    """a connection that does not hold the launch key is dropped and the acceptor keeps accepting; the
    rendezvous directory must be private to this user"""
    import struct
    from pyshepseg_amd import comm as C
    d = tmp_path / 'rv'
    monkeypatch.setenv('SHEPSEG_COMM_DIR', str(d))
    c = C.SocketComm(rank=0, world=1)
    assert (os.stat(d).st_mode & 0o777) == 0o700
    port = c.srv.getsockname()[1]
    for junk in (b'', b'\x00' * 3, struct.pack('<i', 0) + b'x' * 32):
        s = socket.create_connection(('127.0.0.1', port), timeout=10)
        s.recv(16)
        s.sendall(junk)
        s.close()
    assert 0 not in c.inc                                      # nobody was registered as rank 0
    c.send_bytes(np.arange(1000, dtype=np.uint32), 0)          # the real thing still gets through
    assert np.array_equal(np.frombuffer(c.recv_bytes(0, timeout=20), dtype=np.uint32), np.arange(1000))
    c.closing = True
    c.srv.close()
    os.chmod(d, 0o777)
    with pytest.raises(C.CommError, match='not a private directory'):
        C.rendezvousDir()
