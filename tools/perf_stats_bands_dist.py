"""Per-segment statistics of N bands on the row-sharded multi-rank layout: ONE call of the device path with N
entries (distributed.deviceStatsBands, what calcPerSegmentStatsDistributedBands runs under a device communicator)
against N calls with one entry each (distributed.deviceStats, a wrapper over the same driver), on the C5 label raster of `bench.py --workload c5
--gpus N` (4 x 8-pixel blocks, shard boundaries two rows into a block row, so every boundary cuts nCols / 8
segments), (a) world 1 under RCCL, (b) two socket ranks sharing GPU 0 (device buffers staged through the host: that
times the code path, not a second GPU).

    python tools/perf_stats_bands_dist.py [--variant bands,single] [--bands 1,3,6] [--worlds 1,2] [--size 40000]
           [--repeats 6] [--root REPO] [--tag TAG] [--out results.jsonl]
    python tools/perf_stats_bands_dist.py --summarise results.jsonl [more.jsonl ...]
    (a rank: python tools/perf_stats_bands_dist.py --rank TRANSPORT ...the same options)

Every (variant, N) is run once untimed and then --repeats times.  A line of JSON per timed run, printed by rank 0:
wall = the slowest rank's host clock around the call(s), between two barriers (the assembled columns are copied to
the host on rank 0, as in the benchmark); dev = rank 0's PROF_SEGSTATS event counter (the statistics kernels of
the local and the merge part; not the classification, the gather or the exchange).  With N = 1 the two variants
run the same code.  --root imports pyshepseg_amd from another checkout (one without deviceStatsBands runs --variant
single only, and one whose deviceStats still has a driver of its own puts 12 bytes per straddler pixel on the wire):
baseline and candidate are then two processes over the same inputs, to be alternated.  --summarise prints min / median / max per (world, variant, N) and the ratio of the
medians with the baseline's own spread.  The label raster is held whole by every rank, as in the benchmark:
choose --size so that it fits the GPU `world` times."""
import argparse
import ctypes
import json
import os
import secrets
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

BH, BW = 4, 8
SEL = [('mean', 'mean'), ('sd', 'stddev'), ('med', 'median'), ('n', 'pixcount')]
PROF_SEGSTATS = 8


def summarise(paths):
    rows = {}
    for p in paths:
        for line in open(p):
            if line.startswith('{'):
                r = json.loads(line)
                rows.setdefault((r['world'], r['n'], r['variant'], r.get('tag', '')), []).append(r)
    print('%5s %3s %-7s %-10s %4s  %-30s %-30s' % ('world', 'N', 'variant', 'tag', 'runs', 'wall ms min/median/max',
                                                   'device ms min/median/max'))
    med = {}
    for key in sorted(rows):
        w = sorted(r['wall_ms'] for r in rows[key])
        d = sorted(r['dev_ms'] for r in rows[key])
        med[key] = (statistics.median(w), statistics.median(d), w[-1] - w[0], d[-1] - d[0])
        print('%5d %3d %-7s %-10s %4d  %-30s %-30s' % (key + (len(w), '%.1f / %.1f / %.1f' % (w[0], med[key][0], w[-1]),
                                                             '%.2f / %.2f / %.2f' % (d[0], med[key][1], d[-1]))))
    for key in sorted(med):
        if key[2] != 'bands':
            continue
        for other in sorted(med):
            if other[:2] == key[:2] and other[2] == 'single':
                print('world %d N=%d: bands[%s] / single[%s]  wall %.3f (spread of single %.1f ms)  device %.3f (spread of '
                      'single %.2f ms)' % (key[0], key[1], key[3], other[3], med[key][0] / med[other][0], med[other][2],
                                           med[key][1] / max(med[other][1], 1e-9), med[other][3]))


def rank(a, transport):
    os.environ['SHEPSEG_DEVICE'] = '0' if transport == 'socket' else os.environ.get('LOCAL_RANK', '0')
    sys.path.insert(0, a.root)
    from pyshepseg_amd import comm as shpcomm
    from pyshepseg_amd import distributed, tiling, tilingstats, _lib
    variants = a.variant.split(',')
    if 'bands' in variants and not hasattr(distributed, 'deviceStatsBands'):
        raise SystemExit('%s has no deviceStatsBands: run it with --variant single' % a.root)
    counts = [int(x) for x in a.bands.split(',')]
    nbMax = max(counts)
    comm = shpcomm.SocketComm() if transport == 'socket' else shpcomm.RcclComm()
    (r, world) = (comm.rank, comm.world)
    c = _lib.ctx()
    L = c._L
    dcomm = comm if getattr(comm, 'onDevice', False) else shpcomm.HostStagedDev(comm, c)
    N = a.size
    if N % BH or N % BW:
        raise SystemExit('the size must be a multiple of %d' % BW)
    cuts = [0] + [min(N, ((N * (k + 1)) // world) // BH * BH + 2) for k in range(world - 1)] + [N]
    (y0, y1) = (cuts[r], cuts[r + 1])
    ras = tiling.DeviceRaster.synth(11, nbMax, y1 - y0, N, y0=y0, x0=0)
    d_full = ctypes.c_void_p()
    c.check(L.shp_dev_alloc(c.handle, N * N * 4, ctypes.byref(d_full)))
    S = ctypes.c_uint32(0)
    c.check(L.shp_dev_block_labels(c.handle, N, N, BH, BW, d_full, ctypes.byref(S)))
    S = S.value
    d_seg = d_full.value + y0 * N * 4
    h = np.full(S + 1, BH * BW, dtype=np.uint32)
    h[0] = 0
    d_hist = ctypes.c_void_p()
    c.check(L.shp_dev_alloc(c.handle, h.nbytes, ctypes.byref(d_hist)))
    c.check(L.shp_dev_upload(c.handle, d_hist, _lib.ptr(h), h.nbytes))
    hist = ('dev', d_hist.value, S + 1)
    (fast1, nInt1, nFloat1) = tilingstats.makeFastStatsSelection(list(range(len(SEL))), SEL)
    plane = (y1 - y0) * N * 2
    oldSingle = 'shp_dstats_local_dev' in _lib._SIGS        # (a --root from before deviceStats became a wrapper)
    out = open(a.out, 'a') if (a.out and r == 0) else None

    def dev_ms(reset):
        ms = (ctypes.c_double * 16)()
        cn = (ctypes.c_uint64 * 16)()
        c.check(L.shp_prof_get(c.handle, ms, cn, 16, int(reset)))
        return ms[PROF_SEGSTATS]

    def run(variant, nb):
        """-> (pixels counted by the last band's pixcount column on rank 0, straddler pixels, exchanged bytes)"""
        if variant == 'bands':
            sels = [(b + 1, [('b%d_%s' % (b + 1, s[0]),) + s[1:] for s in SEL]) for b in range(nb)]
            (fast, _bo, nInt, nFloat) = tilingstats.makeBandStatsSelection(sels)
            (ic, _fc, _ns, nPix, nBytes) = distributed.deviceStatsBands(
                c, dcomm, d_seg, [ras.ptr + b * plane for b in range(nb)], 2, y1 - y0, N, hist, fast, [len(SEL)] * nb,
                [0] * nb, [0] * nb, nInt, nFloat, -9999, fetch=(r == 0))
            return (int(ic[nInt - 1].sum()) if r == 0 else None), nPix, nBytes
        for b in range(nb):
            (ic, _fc, _ns, nPix) = distributed.deviceStats(c, dcomm, d_seg, ras.ptr + b * plane, 2, y1 - y0, N, hist, fast1,
                                                           nInt1, nFloat1, -9999, None, fetch=(r == 0))
        return (int(ic[nInt1 - 1].sum()) if r == 0 else None), nPix, (12 if oldSingle else 4 + 2) * nb * nPix

    if r == 0:
        print('world %d (%s): %d x %d labels, %d segments, %d bands of uint16, rows per rank %s'
              % (world, getattr(dcomm, 'transport', type(dcomm).__name__), N, N, S, nbMax,
                 [cuts[k + 1] - cuts[k] for k in range(world)]), flush=True)
    for nb in counts:
        for variant in variants:
            for rep in range(-1, a.repeats):                    # (-1: the untimed run)
                c.check(L.shp_sync(c.handle))
                comm.barrier()
                dev_ms(True)
                t = time.perf_counter()
                (npx, nPix, nBytes) = run(variant, nb)
                c.check(L.shp_sync(c.handle))
                comm.barrier()
                wall = comm.max_f64((time.perf_counter() - t) * 1e3)
                dev = dev_ms(True)
                if r != 0:
                    continue
                assert npx == N * N, (npx, N * N)
                if rep < 0:
                    continue
                line = json.dumps(dict(world=world, variant=variant, n=nb, size=N, rep=rep, tag=a.tag,
                                       wall_ms=round(wall, 2), dev_ms=round(dev, 3), straddler_pixels=nPix,
                                       exchange_bytes=nBytes))
                print(line, flush=True)
                if out:
                    out.write(line + '\n')
                    out.flush()
    comm.barrier()
    c.check(L.shp_dev_free(c.handle, d_hist))
    c.check(L.shp_dev_free(c.handle, d_full))
    ras.free()
    comm.close()


def launch(world, transport, argv):
    """`world` rank processes of this program; the first that fails stops the others"""
    nonce = secrets.token_hex(8)
    tmp = tempfile.mkdtemp(prefix='perf_stats_bands_dist_')
    procs = []
    for r in range(world):
        env = dict(os.environ, SHEPSEG_LAUNCH_NONCE=nonce, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT='0', SHEPSEG_COMM_DIR=os.path.join(tmp, 'comm'))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), '--rank', transport] + argv, env=env))
    bad = None
    try:
        while bad is None and any(p.poll() is None for p in procs):
            bad = next((p.returncode for p in procs if p.poll() not in (None, 0)), None)
            time.sleep(0.1)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    bad = bad if bad is not None else next((p.returncode for p in procs if p.returncode != 0), None)
    if bad is not None:
        raise SystemExit('a rank exited with %d' % bad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rank', default=None, metavar='TRANSPORT')
    ap.add_argument('--variant', default='bands,single')
    ap.add_argument('--bands', default='1,3,6')
    ap.add_argument('--worlds', default='1,2')
    ap.add_argument('--size', type=int, default=40000)
    ap.add_argument('--repeats', type=int, default=6)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default=None)
    ap.add_argument('--summarise', nargs='+')
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    if a.rank:
        return rank(a, a.rank)
    argv = ['--variant', a.variant, '--bands', a.bands, '--size', str(a.size), '--repeats', str(a.repeats), '--root', a.root,
            '--tag', a.tag] + (['--out', a.out] if a.out else [])
    for world in [int(w) for w in a.worlds.split(',')]:
        launch(world, 'rccl' if world == 1 else 'socket', argv)


if __name__ == '__main__':
    main()
