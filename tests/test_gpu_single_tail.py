"""The later passes of the single-pixel stage in one workgroup (csrc/elim_single.h k_single_tail: up to twenty passes,
lists above and below one round of its 1024 threads, the compacting and the non-compacting branch) on the tiles of
tests/single_tail_cases.py, whose properties tests/test_single_tail_census.py pins on the CPU.  Every case runs
shp_segment_tile in a fresh child and compares labels, maxSegId and the number of single pixels eliminated with the
oracle exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

import single_tail_cases as stc
from conftest import ROOT

pytestmark = pytest.mark.gpu

ABNORMAL = []       # the first child that crashed or timed out (no child is started after it)


@pytest.mark.parametrize('name', sorted(stc.CASES))
def test_tail_matches_oracle(name, oracle, tmp_path):
    if ABNORMAL:
        pytest.fail('not started: child %s ended abnormally' % ABNORMAL[0])
    img, cen, nullv, four = stc.build(name)
    want = oracle.segment_tile(img, cen, stc.MINSEG, stc.MSD, nullv, four)
    out = str(tmp_path / 'out.npz')
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'single_tail_cases.py'), name, out], cwd=ROOT,
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        ABNORMAL.append('%s (timeout)' % name)
        pytest.fail('child %s timed out' % name)
    if p.returncode < 0 or p.returncode in (134, 139):
        ABNORMAL.append('%s (exit %d)' % (name, p.returncode))
    assert p.returncode == 0, 'child %s exit %d:\n%s' % (name, p.returncode, p.stderr[-3000:])
    with np.load(out) as got:
        print('%s: singles eliminated %d, maxSegId %d' % (name, int(got['singles']), int(got['max_seg_id'])))
        assert int(got['singles']) == want['singlePixelsEliminated'] > 0
        assert int(got['small']) == want['smallSegmentsEliminated'] == 0
        assert int(got['max_seg_id']) == want['maxSegId']
        assert np.array_equal(got['seg'], want['segimg'])
