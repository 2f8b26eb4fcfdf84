"""The latency-bound kernels of several tiles in one launch (csrc/walkbatch.h): a tiled run of 24 tiles of four
sizes under one walker stream, two, and the default environment, both connectivities, against the oracle.

4-connected, 23 tiles hold 1-3 components above the depth-first cut's cap and tile (0, 0) holds none: its worker
skips the replay while the others batch.  8-connected, all 24 hold 1-3.  Every tile eliminates at least 21 small
segments, so every tile runs a pass loop.  A replay job has ceil(components / SHEPSEG_DFS_PER_WG) workgroups, so at
the default of 8 every replay job here is ONE workgroup: these cases pin the batcher and the batch kernels' job
lookup for such jobs only; jobs of several workgroups, other pass-loop group sizes and the caps are the business of
tests/test_gpu_walk_batch_uneven.py, and tests/walk_batch_cases.census('even', ...) recounts the figures above.
The library reads its knobs once per process, so every setting runs in a fresh child (tests/walk_batch_worker.py),
one at a time; after a child that ended abnormally (here or in the sibling file) none is started."""
import os
import subprocess
import sys

import numpy as np
import pytest

import seg_cases
import walk_batch_cases as wbc
import walk_batch_worker as wbw
from conftest import ROOT

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, 'tests', 'walk_batch_worker.py')
WORKERS = 8
_abnormal = wbc.ABNORMAL     # the first child that crashed or timed out, shared with the sibling file

SETTINGS = [('walk_streams_1', {'SHEPSEG_WALK_STREAMS': '1'}), ('walk_streams_2', {'SHEPSEG_WALK_STREAMS': '2'}),
            ('default', {})]


@pytest.fixture(scope='module')
def want(oracle):
    img, centres = wbw.image()
    cache = {}

    def get(four):
        if four not in cache:
            cache[four] = seg_cases.oracle_tiled(oracle, img, centres, wbw.TILE, wbw.OVERLAP, wbw.MINSEG, wbw.MSD,
                                                 None, four)
        return cache[four]
    return get


def test_expected_mosaics(want):
    """the case is what its description says: the oracle's segment counts"""
    assert want(True)[1] == 401 and want(False)[1] == 305


@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
@pytest.mark.parametrize('setting,env', SETTINGS, ids=[s[0] for s in SETTINGS])
def test_batched_tiles_match_oracle(setting, env, four, want, tmp_path):
    if _abnormal:
        pytest.fail('not started: child %s ended abnormally' % _abnormal[0])
    out = str(tmp_path / 'out.npz')
    child_env = dict(os.environ, **env)
    if not env:
        child_env.pop('SHEPSEG_WALK_STREAMS', None)
    name = '%s/%s' % (setting, 'four' if four else 'eight')
    try:
        p = subprocess.run([sys.executable, WORKER, out, str(int(four)), str(WORKERS)], env=child_env, cwd=ROOT,
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _abnormal.append('%s (timeout)' % name)
        pytest.fail('child %s timed out' % name)
    if p.returncode < 0 or p.returncode in (134, 139):
        _abnormal.append('%s (exit %d)' % (name, p.returncode))
    assert p.returncode == 0, 'child %s exit %d:\n%s' % (name, p.returncode, p.stderr[-3000:])
    wseg, wmx, whist = want(four)
    with np.load(out) as got:
        stats = [int(v) for v in got['stats']]
        print('%s: replay launches %d jobs %d largest %d; pass loop launches %d jobs %d largest %d' % ((name,) + tuple(stats)))
        assert int(got['max_seg_id']) == wmx
        assert np.array_equal(got['seg'], wseg)
        assert np.array_equal(got['hist'], whist)
    r_launch, r_jobs, r_big, l_launch, l_jobs, l_big = stats
    assert r_jobs == (23 if four else 24)
    assert l_jobs == 24
    assert 1 <= r_launch <= r_jobs and 1 <= l_launch <= l_jobs
    if setting == 'walk_streams_1':
        # with one walker stream no worker passes its submit while a launch is out: the pending jobs accumulate
        # and the next leader takes them all
        assert r_big >= 2 and l_big >= 2
