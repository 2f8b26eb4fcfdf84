"""Timings of the multi-rank file-to-file entry point (distributed.doTiledShepherdSegmentationDistributed) on a
synthetic N x N, 6-band uint16 .npy (synthimg v1, written first to a temporary directory), default tile and
overlap, fixedKMeansInit:

  one GPU  tiling.doTiledShepherdSegmentation from the .npy to a .npy (mosaic, histogram, overview layers);
  W = 1    the entry point with an RcclComm;
  W = 2, 4 socket ranks sharing GPU 0 (the shape of tests/test_gpu_dist_output.py).

Per rank: read + upload of its rows, runDistributed (the rest of the wall time), the mosaic write and the overview
layers.  Every run's files are checked against the one-GPU run's.

    python tools/perf_dist_output.py [N=16000] [W=2,4]
    (a rank: python tools/perf_dist_output.py --rank IMG.npy OUT.npy TRANSPORT)"""
import json
import os
import secrets
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def rank(img, out, transport):
    os.environ['SHEPSEG_DEVICE'] = '0' if transport == 'socket' else os.environ.get('LOCAL_RANK', '0')
    from pyshepseg_amd import comm as shpcomm
    from pyshepseg_amd import distributed, tiling
    comm = shpcomm.SocketComm() if transport == 'socket' else shpcomm.RcclComm()
    cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=16)
    comm.barrier()
    t0 = time.time()
    r = distributed.doTiledShepherdSegmentationDistributed(img, out, comm=comm, fixedKMeansInit=True,
                                                           concurrencyCfg=cfg)
    wall = time.time() - t0
    d = r.timings.makeSummaryDict()
    part = {k: round(d.get(k, {'total': 0.0})['total'], 3) for k in ('reading', 'writing', 'overviews')}
    part['runDistributed'] = round(d['walltime']['total'] - sum(part.values()), 3)
    part.update(rank=comm.rank, wall=round(wall, 3), tiles=list(r.tileRange), rows=list(r.outRows),
                stitch=r.stitchMode, maxSegId=r.maxSegId)
    print(json.dumps(part), flush=True)
    comm.close()


def launch(world, transport, img, out, tmp):
    nonce = secrets.token_hex(8)
    procs = []
    for r in range(world):
        env = dict(os.environ, SHEPSEG_LAUNCH_NONCE=nonce, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT='0', SHEPSEG_COMM_DIR=os.path.join(tmp, 'comm_' + nonce))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), '--rank', img, out, transport],
                                      env=env, stdout=subprocess.PIPE, text=True))
    rows = []
    for p in procs:
        (so, _se) = p.communicate(timeout=900)
        if p.returncode != 0:
            raise SystemExit('a rank exited with %d' % p.returncode)
        rows.append(json.loads(so.strip().splitlines()[-1]))
    return rows


def same(a, b):
    names = sorted(f for f in os.listdir(os.path.dirname(a)) if f.startswith(os.path.basename(a)[:-4]))
    for f in names:
        other = os.path.join(os.path.dirname(b), os.path.basename(b)[:-4] + f[len(os.path.basename(a)[:-4]):])
        if not np.array_equal(np.load(os.path.join(os.path.dirname(a), f)), np.load(other)):
            return False
    return bool(names)


def main(N, worlds):
    from pyshepseg_amd import tiling
    tmp = tempfile.mkdtemp(prefix='perf_dist_output_')
    try:
        img = os.path.join(tmp, 'img.npy')
        t0 = time.time()
        ras = tiling.DeviceRaster.synth(11, 6, N, N)
        a = np.lib.format.open_memmap(img, mode='w+', dtype=np.uint16, shape=(6, N, N))
        a[...] = ras.toArray()
        a.flush()
        del a
        ras.free()
        print('input %d x %d x 6 uint16 written in %.1f s' % (N, N, time.time() - t0), flush=True)
        os.makedirs(os.path.join(tmp, 'one'))
        cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=16)
        t0 = time.time()
        r = tiling.doTiledShepherdSegmentation(img, os.path.join(tmp, 'one', 'out.npy'), fixedKMeansInit=True,
                                               concurrencyCfg=cfg)
        one = time.time() - t0
        d = r.timings.makeSummaryDict()
        print(json.dumps({'one_gpu_wall': round(one, 3), 'maxSegId': r.maxSegId,
                          'writing': round(d.get('writing', {'total': 0})['total'], 3)}), flush=True)
        tiling.clearDeviceCache()
        for (world, transport) in [(1, 'rccl')] + [(w, 'socket') for w in worlds]:
            d = os.path.join(tmp, 'w%d' % world)
            os.makedirs(d)
            rows = launch(world, transport, img, os.path.join(d, 'out.npy'), tmp)
            ok = same(os.path.join(tmp, 'one', 'out.npy'), os.path.join(d, 'out.npy'))
            print(json.dumps({'world': world, 'transport': transport, 'files_equal_one_gpu': ok,
                              'wall': max(q['wall'] for q in rows), 'ranks': rows}), flush=True)
            shutil.rmtree(d)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--rank':
        rank(*sys.argv[2:5])
    else:
        N = int(sys.argv[1]) if len(sys.argv) > 1 else 16000
        worlds = [int(w) for w in sys.argv[2].split(',')] if len(sys.argv) > 2 else [2, 4]
        main(N, worlds)
