"""Helpers of the multi-rank stitch tests (no tests here): the random rasters of the parallel-stitch fuzz,
shard range lists a test chooses itself (checked against shardTiles' invariant), the places of the partial
redo's first kept tile `bad` relative to the rank boundaries, and a rank launcher that stops every rank when
one of them fails or runs out of time."""
import itertools
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class _Ds(object):
    def __init__(self, ys, xs):
        self.RasterYSize, self.RasterXSize = ys, xs


def tileInfoOf(nr, nc, tile, ov):
    from pyshepseg_amd import tiling
    return tiling.getTilesForFile(_Ds(nr, nc), tile, ov)


# ------------------------------------------------------------------------------------------
# the fuzz recipe of test_parallel_stitch_fuzz_in_process
# ------------------------------------------------------------------------------------------
def fuzzCase(seed, oracle):
    """Small random raster with many tiles: a dict of the image, its tiling and the model."""
    from pyshepseg_amd import shepseg
    rng = np.random.default_rng(seed)
    (nr, nc) = (int(rng.integers(120, 260)), int(rng.integers(120, 260)))
    img = oracle.synthimg(100 + seed, 3, nr, nc)
    if seed % 2:
        img[:, : int(rng.integers(1, 9)), :] = 65535
    (tile, ov) = [(48, 32), (64, 24), (80, 40), (56, 16)][seed % 4]
    null = 65535 if seed % 2 else None
    xs = shepseg._sample_rows(img, 100, null)
    init = shepseg.diagonalClusterCentres(xs, 6).astype(np.float64)
    centres, _l, _n = oracle.kmeans_fit(xs.astype(np.float64), init)
    msd = float(shepseg.autoMaxSpectralDiff(shepseg.KMeansModel(centres), 'auto', 50))
    ti = tileInfoOf(nr, nc, tile, ov)
    return dict(seed=seed, img=img, nr=nr, nc=nc, tile=tile, ov=ov, null=null, four=bool(seed % 3),
                centres=centres, msd=msd, minseg=14, ncols=ti.ncols, ntiles=ti.ncols * ti.nrows)


def runInProcess(case, oracle, mode):
    """One rank, the oracle engine: (output, DistResult)."""
    sys.path.insert(0, HERE)
    from dist_oracle_engine import OracleEngine
    from pyshepseg_amd import comm as shpcomm
    from pyshepseg_amd import distributed, shepseg
    eng = OracleEngine(case['img'], oracle)
    r = distributed.runDistributed(
        eng, shpcomm.LocalComm(), case['nr'], case['nc'], case['tile'], case['ov'], minSegmentSize=case['minseg'],
        maxSpectralDiff='auto', imgNullVal=case['null'], fourConnected=case['four'],
        kmeansObj=shepseg.KMeansModel(case['centres']), stitchMode=mode)
    return eng.out.copy(), r


def badTile(case, oracle):
    """The first tile the partial redo keeps (`bad`: the chain is redone from the tile after it), or None
    when the one-rank parallel stitch keeps everything or redoes everything."""
    _out, r = runInProcess(case, oracle, 'parallel')
    if r.stitchMode != 'parallel->sequential' or r.chainStepsRedone >= case['ntiles']:
        return None
    return case['ntiles'] - 1 - r.chainStepsRedone


def sequentialReference(case, oracle):
    """The oracle's tiles stitched sequentially: (mosaic, maxSegId, histogram)."""
    img = case['img']
    tiles, ntc, ntr = oracle.get_tiles(case['nr'], case['nc'], case['tile'], case['ov'])
    local = {}
    for (c, r), (x, y, xs, ys) in tiles.items():
        sub = np.ascontiguousarray(img[:, y:y + ys, x:x + xs])
        local[(c, r)] = oracle.segment_tile(sub, case['centres'], case['minseg'], case['msd'], case['null'],
                                            case['four'])['segimg']
    return oracle.stitch_tiles(local, tiles, ntc, ntr, case['nr'], case['nc'], case['ov'])


def checkRanksAgainst(reference, parts, what):
    """every rank's maxSegId, histogram and the output rows it wrote == reference (mosaic, maxSegId, histogram);
    together the ranks' rows cover the mosaic"""
    (want, mx, hist) = reference
    got = np.zeros_like(want)
    cover = np.zeros(want.shape[0], dtype=bool)
    for (r, q) in enumerate(parts):
        assert int(q['maxSegId']) == int(mx), (what, r, int(q['maxSegId']), int(mx))
        assert np.array_equal(q['hist'], hist), (what, r)
        (lo, hi) = (int(q['outLo']), int(q['outHi']))
        out = q['out']
        written = out != 0                       # a rank writes its tiles' windows only, the rest stays 0
        assert np.array_equal(out[written], want[lo:hi][written]), (what, r)
        got[lo:hi] = np.maximum(got[lo:hi], out)
        cover[lo:hi] = True
    assert cover.all(), what
    assert np.array_equal(got, want), what


def saveCase(case, path):
    """The case in the form of a stitch fixture (tests/dist_worker.py reads it)."""
    np.savez(path, img=case['img'], tile_size=case['tile'], overlap=case['ov'], min_seg=case['minseg'],
             msd=case['msd'], null_val=0 if case['null'] is None else case['null'],
             has_null=int(case['null'] is not None), four=int(case['four']), centres=case['centres'])


# ------------------------------------------------------------------------------------------
# shard ranges
# ------------------------------------------------------------------------------------------
def shardProblems(ranges, ncols, nt):
    """What is wrong with a list of [t0, t1) tile ranges, one per rank, against shardTiles' invariant:
    contiguous, complete and in order; every rank with tiles that has a successor with tiles holds at least
    ncols of them (so a tile's top neighbour is local or in the previous rank).  Empty ranks are allowed."""
    bad = []
    if [t for (a, b) in ranges for t in range(a, b)] != list(range(nt)) or any(b < a for (a, b) in ranges):
        bad.append('not contiguous, complete and ordered: %s' % (ranges,))
    ne = [(a, b) for (a, b) in ranges if b > a]
    for (a, b) in ne[:-1]:
        if b - a < ncols:
            bad.append('range %s has a successor but fewer than %d tiles' % ((a, b), ncols))
    return bad


def checkShardRanges(ranges, ncols, nt):
    probs = shardProblems(ranges, ncols, nt)
    assert not probs, probs


def checkNeighboursDelivered(ti, ranges, ov):
    """Every tile's top and left neighbours are in its own range or in the previous range's boundary plan."""
    from pyshepseg_amd import distributed
    ne = [i for i, (a, b) in enumerate(ranges) if b > a]
    for pos, r in enumerate(ne):
        (a, b) = ranges[r]
        got = set()
        if pos > 0:
            got = {(k, col, row) for (k, col, row, _h, _w) in
                   distributed.boundaryPlan(ti, ranges, ne[pos - 1], ov)}
        for t in range(a, b):
            (col, row) = (t % ti.ncols, t // ti.ncols)
            if row > 0 and not (a <= t - ti.ncols < b):
                assert ('b', col, row - 1) in got, (ranges, t)
            if col > 0 and not (a <= t - 1 < b):
                assert ('r', col - 1, row) in got, (ranges, t)


def validRanges(ncols, nt, world):
    """Every range list of `world` ranks over nt tiles that keeps the invariant."""
    out = []
    for cuts in itertools.combinations_with_replacement(range(nt + 1), world - 1):
        edges = (0,) + cuts + (nt,)
        ranges = [(edges[i], edges[i + 1]) for i in range(world)]
        if not shardProblems(ranges, ncols, nt):
            out.append(ranges)
    return out


def _nonEmpty(ranges):
    return [(i, a, b) for i, (a, b) in enumerate(ranges) if b > a]


def _lastOfSender(ranges, bad):
    """`bad` is the last tile of a rank that has a successor with tiles (it redoes nothing, sends on)"""
    ne = _nonEmpty(ranges)
    return any(b - 1 == bad for (_i, _a, b) in ne[:-1])


def _emptyBetween(ranges):
    ne = [i for (i, _a, _b) in _nonEmpty(ranges)]
    return any(a == b and ne[0] < i < ne[-1] for i, (a, b) in enumerate(ranges))


def _midRowStart(ranges, ncols):
    return any(a % ncols != 0 for (_i, a, _b) in _nonEmpty(ranges)[1:])


# where `bad` lies relative to the rank boundaries (and the other shapes a partial redo must survive)
PLACEMENTS = {
    'bad_last_of_sender': lambda rs, bad, ncols: _lastOfSender(rs, bad),
    'bad_last_of_sender_midrow': lambda rs, bad, ncols: any(
        b - 1 == bad and b % ncols != 0 for (_i, _a, b) in _nonEmpty(rs)[:-1]),
    'bad_first_of_rank': lambda rs, bad, ncols: any(a == bad for (_i, a, _b) in _nonEmpty(rs)[1:]),
    'bad_mid_range': lambda rs, bad, ncols: any(a < bad < b - 1 for (_i, a, b) in _nonEmpty(rs)),
    'bad_on_last_rank': lambda rs, bad, ncols: _nonEmpty(rs)[-1][1] <= bad,
    'rank_all_redone': lambda rs, bad, ncols: any(a > bad for (_i, a, _b) in _nonEmpty(rs)),
    'empty_rank': lambda rs, bad, ncols: _emptyBetween(rs),
    'midrow_boundary': lambda rs, bad, ncols: _midRowStart(rs, ncols),
}


def placementsOf(ranges, bad, ncols):
    return sorted(k for (k, f) in PLACEMENTS.items() if f(ranges, bad, ncols))


def pickRanges(ncols, nt, world, bad):
    """One valid range list per placement that exists at this world size (a list of (placement, ranges),
    distinct range lists only).  Among the candidates the ones that also put `bad` at a sender's last tile
    come first, then the most even."""
    cands = validRanges(ncols, nt, world)

    def key(rs):
        return (not _lastOfSender(rs, bad), max(b - a for (a, b) in rs) - min(b - a for (a, b) in rs), rs)
    cands.sort(key=key)
    picked = []
    for name, f in PLACEMENTS.items():
        if any(f(rs, bad, ncols) for (_n, rs) in picked):
            continue
        for rs in cands:
            if f(rs, bad, ncols):
                picked.append((name, rs))
                break
    return picked


def encodeRanges(ranges):
    return ','.join('%d:%d' % (a, b) for (a, b) in ranges)


def decodeRanges(s):
    return [tuple(int(v) for v in p.split(':')) for p in s.split(',')]


# ------------------------------------------------------------------------------------------
# rank launcher
# ------------------------------------------------------------------------------------------
def runRanks(world, argv, tmp_path, timeout, extra_env=None, base_env=None):
    """Start `world` rank processes with the environment a launcher sets.  Each has `timeout` seconds; the
    first one that exits non-zero or runs out of time stops every rank and fails the test (never retried).
    Returns the ranks' stderr."""
    import secrets
    nonce = secrets.token_hex(8)
    logs = []
    procs = []
    try:
        for r in range(world):
            env = dict(os.environ, SHEPSEG_LAUNCH_NONCE=nonce, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world),
                       MASTER_ADDR='127.0.0.1', MASTER_PORT='0', SHEPSEG_COMM_DIR=str(tmp_path / 'comm'))
            env.update(base_env or {})
            env.update(extra_env or {})
            err = open(str(tmp_path / ('rank%d.stderr' % r)), 'w+')
            logs.append(err)
            procs.append(subprocess.Popen([sys.executable] + argv, env=env, stdout=subprocess.DEVNULL,
                                          stderr=err, text=True))
        deadline = time.monotonic() + timeout
        failed = None
        while failed is None and any(p.poll() is None for p in procs):
            for (r, p) in enumerate(procs):
                if p.poll() not in (None, 0):
                    failed = 'rank %d exited with %d' % (r, p.returncode)
                    break
            else:
                if time.monotonic() > deadline:
                    failed = 'ranks still running after %d s' % timeout
                else:
                    time.sleep(0.05)
        if failed is None:
            bad = [(r, p.returncode) for (r, p) in enumerate(procs) if p.returncode != 0]
            if bad:
                failed = 'rank %d exited with %d' % bad[0]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    errs = []
    for f in logs:
        f.seek(0)
        errs.append(f.read())
        f.close()
    assert failed is None, '%s\n%s' % (failed, '\n'.join('--- rank %d:\n%s' % (r, e[-3000:])
                                                         for (r, e) in enumerate(errs) if e))
    return errs
