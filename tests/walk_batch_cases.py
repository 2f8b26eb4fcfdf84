"""What the walker-batch tests know about their rasters without a GPU: per tile window, the number of components
above the depth-first cut's cap (one replay job of ceil(n / SHEPSEG_DFS_PER_WG) workgroups each, none for n = 0)
and whether the tile eliminates a small segment (then it runs a pass loop); and the one-at-a-time child runner the
GPU tests share."""
import os
import subprocess
import sys

import numpy as np

import clump_shape_cases
import walk_batch_worker as wbw
from conftest import ROOT

WORKER = os.path.join(ROOT, 'tests', 'walk_batch_worker.py')
DFS_MAX_BLOCKS = 256        # csrc/clump.h: workgroups of one replay job at the most
DFS_MAX_JOBS = 16           # csrc/clump.h: replay jobs of one launch at the most
DFS_WAVES = 8               # csrc/clump.h: the default SHEPSEG_DFS_PER_WG
SMALL_BLOCKS = 64           # csrc/elim_small.h: the default SHEPSEG_SMALL_BLOCKS
ABNORMAL = []               # the first child that crashed or timed out (no child is started after it)

_census = {}


def census(oracle, raster, four):
    """(components above the cap, small segments eliminated) per tile, two lists in sorted tile-key order"""
    key = (raster, bool(four))
    if key not in _census:
        img, centres = wbw.IMAGES[raster]()
        tiles, _ntc, _ntr = oracle.get_tiles(wbw.NR, wbw.NC, wbw.TILE, wbw.OVERLAP)
        comps, elim = [], []
        for k in sorted(tiles):
            (x, y, xs, ys) = tiles[k]
            sub = np.ascontiguousarray(img[:, y:y + ys, x:x + xs])
            cl = oracle.kmeans_assign(sub, centres).astype(np.int32)
            comps.append(len(clump_shape_cases.cut_components(cl, four)))
            elim.append(int(oracle.segment_tile(sub, centres, wbw.MINSEG, wbw.MSD, None, four)['smallSegmentsEliminated']))
        _census[key] = (comps, elim)
    return _census[key]


def job_blocks(comps, per_wg):
    """workgroups of every replay job: the tiles with a component above the cap, in the census' order"""
    return [min(DFS_MAX_BLOCKS, -(-n // per_wg)) for n in comps if n > 0]


def expected_replay(comps, per_wg):
    """(replay jobs, sum of replay workgroups) of a tiled run"""
    b = job_blocks(comps, per_wg)
    return len(b), sum(b)


def run_child(name, env, four, workers, raster, out):
    """One fresh child under `env` on top of this process' environment (a knob that `env` does not name is unset),
    120 s at the most; returns the loaded .npz as a dict.  Fails without starting anything after a child that
    ended abnormally."""
    import pytest
    if ABNORMAL:
        pytest.fail('not started: child %s ended abnormally' % ABNORMAL[0])
    child_env = dict(os.environ)
    for k in ('SHEPSEG_WALK_STREAMS', 'SHEPSEG_DFS_PER_WG', 'SHEPSEG_SMALL_BLOCKS', 'SHEPSEG_SMALL_MAX',
              'SHEPSEG_SHARED_STREAMS'):
        child_env.pop(k, None)
    child_env.update(env)
    try:
        p = subprocess.run([sys.executable, WORKER, out, four, str(workers), raster], env=child_env, cwd=ROOT,
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        ABNORMAL.append('%s (timeout)' % name)
        pytest.fail('child %s timed out' % name)
    if p.returncode < 0 or p.returncode in (134, 139):
        ABNORMAL.append('%s (exit %d)' % (name, p.returncode))
    assert p.returncode == 0, 'child %s exit %d:\n%s' % (name, p.returncode, p.stderr[-3000:])
    with np.load(out) as got:
        return {k: got[k] for k in got.files}
