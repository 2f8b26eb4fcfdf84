"""The spectra of the segments above 64 pixels (csrc/elim_small.h k_spectra_big) in tiled runs of the raster of
tests/spectra_batch_cases.py, whose tiles hold segments of every kind that kernel treats differently: 65, 512 and 513
pixels, pieces of ~10 000 pixels, each with values near 65535 and below 1500, so on both sides of the 2^24 bound of its
exact phase (tests/test_spectra_batch_census.py pins that on the CPU).  Blobs below minSegmentSize across the
segments' borders make the labels depend on the sums.  Every case compares labels, histogram and maxSegId of the mosaic
with the oracle exactly.

What a case pins:
  one_stream   (both connectivities) one walker stream: the pass loops that read the sums of several tiles may share
               a launch
  unshared     SHEPSEG_SHARED_STREAMS=0: every tile on its worker's own stream
  bands10      ten bands: two band groups at SPECTRA_BG 8
  mixed        a uint8 and a uint16 run at once in one process: two instances of the kernels side by side
The library reads its knobs once per process, so every case runs in a fresh child, one at a time; after a child
that ended abnormally none is started."""
import os
import subprocess
import sys

import numpy as np
import pytest

import seg_cases
import spectra_batch_cases as sbc
from conftest import ROOT

pytestmark = pytest.mark.gpu

WORKERS = 8
ABNORMAL = []
KNOBS = ('SHEPSEG_WALK_STREAMS', 'SHEPSEG_SHARED_STREAMS', 'SHEPSEG_FILL_MAX', 'SHEPSEG_SMALL_BLOCKS', 'SHEPSEG_SMALL_MAX')
# (id, environment, mode)
CASES = [
    ('one_stream-four', {'SHEPSEG_WALK_STREAMS': '1'}, 'four'),
    ('one_stream-eight', {'SHEPSEG_WALK_STREAMS': '1'}, 'eight'),
    ('unshared', {'SHEPSEG_SHARED_STREAMS': '0'}, 'four'),
    ('bands10', {'SHEPSEG_WALK_STREAMS': '1'}, 'bands10'),
    ('mixed', {'SHEPSEG_WALK_STREAMS': '1'}, 'mixed'),
]
RUNS = {'four': [('uint16', 6, True)], 'eight': [('uint16', 6, False)], 'bands10': [('uint16', 10, True)],
        'mixed': [('uint8', 6, True), ('uint16', 6, True)]}


@pytest.fixture(scope='module')
def want(oracle):
    cache = {}

    def get(dtype, nb, four):
        if (dtype, nb, four) not in cache:
            img, cen = sbc.image(dtype, nb)
            cache[(dtype, nb, four)] = seg_cases.oracle_tiled(oracle, img, cen, sbc.TILE, sbc.OVERLAP, sbc.MINSEG,
                                                              sbc.MSD, None, four)
        return cache[(dtype, nb, four)]
    return get


def run_child(name, env, mode, out):
    if ABNORMAL:
        pytest.fail('not started: child %s ended abnormally' % ABNORMAL[0])
    child_env = dict(os.environ)
    for k in KNOBS:
        child_env.pop(k, None)
    child_env.update(env)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'spectra_batch_cases.py'), out, mode,
                            str(WORKERS)], env=child_env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        ABNORMAL.append('%s (timeout)' % name)
        pytest.fail('child %s timed out' % name)
    if p.returncode < 0 or p.returncode in (134, 139):
        ABNORMAL.append('%s (exit %d)' % (name, p.returncode))
    assert p.returncode == 0, 'child %s exit %d:\n%s' % (name, p.returncode, p.stderr[-3000:])
    with np.load(out) as got:
        return {k: got[k] for k in got.files}


@pytest.mark.parametrize('name,env,mode', CASES, ids=[c[0] for c in CASES])
def test_batched_spectra_match_oracle(name, env, mode, want, tmp_path):
    got = run_child(name, env, mode, str(tmp_path / 'out.npz'))
    l_launch, l_jobs, l_big = [int(v) for v in got['stats'][3:6]]
    print('%s: pass-loop launches %d jobs %d largest batch %d' % (name, l_launch, l_jobs, l_big))
    for (i, (dtype, nb, four)) in enumerate(RUNS[mode]):
        wseg, wmx, whist = want(dtype, nb, four)
        assert int(got['max_seg_id%d' % i]) == wmx
        assert np.array_equal(got['seg%d' % i], wseg)
        assert np.array_equal(got['hist%d' % i], whist)
    assert l_jobs == 4 * len(RUNS[mode])          # every tile ran a pass loop
    # (how many tiles share a pass-loop launch depends on when they arrive: printed, not asserted; k_spectra_big
    #  runs per tile on its fill stream either way)
    assert 1 <= l_launch <= l_jobs and 1 <= l_big <= l_jobs
    if name == 'unshared':
        assert (l_launch, l_big) == (l_jobs, 1)
