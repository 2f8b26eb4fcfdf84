"""The instances of the pass loop (csrc/elim_small.h k_small_loop<NB, CONN, DIAG>): every case of
tests/small_spec_cases.py segments its tile on the GPU, compares labels, histogram and maxSegId exactly with the
oracle and proves through shp_small_loop_instances which instance its one-job launch took.  The census of the
rasters -- passes in every range of pairs per source, both forms of the merge step, both branches of the size-table
scan -- is tests/test_small_spec_census.py, on the CPU.  The mixed batch runs in a child (the library reads its
knobs once per process): a 4-connected and an 8-connected tiled run of a six-band raster at once on one walker
stream."""
import ctypes

import numpy as np
import pytest

import seg_cases
import small_spec_cases as ssc
import small_spec_worker as ssw
import walk_batch_cases as wbc
import walk_batch_worker as wbw

pytestmark = pytest.mark.gpu


def _instances(reset):
    from pyshepseg_amd import _lib
    out = np.zeros(5, dtype=np.uint64)
    assert _lib.lib().shp_small_loop_instances(out.ctypes.data_as(ctypes.c_void_p), int(reset)) == 0
    return [int(v) for v in out]


def _run(oracle, nb, four, minseg, inst, scan=False):
    from pyshepseg_amd import shepseg
    img, centres, msd = ssc.tile(oracle, nb, scan)
    want = ssc.oracle_run(oracle, nb, four, minseg, scan)
    _instances(True)
    r = shepseg.doShepherdSegmentation(img, minSegmentSize=minseg, maxSpectralDiff=msd, fourConnected=four,
                                       kmeansObj=shepseg.KMeansModel(centres))
    got = _instances(False)
    print('launches per instance (generic, 6/4, 6/8, 10/4, 10/8): %s' % got)
    assert int(r.segimg.max()) == int(want['segimg'].max())
    assert np.array_equal(r.segimg, want['segimg'])
    assert np.array_equal(np.bincount(r.segimg.ravel()), np.bincount(want['segimg'].ravel()))
    assert r.smallSegmentsEliminated == want['smallSegmentsEliminated']
    assert got == [1 if i == inst else 0 for i in range(5)]      # one launch, on the intended instance


@pytest.mark.parametrize('cid,nb,four,minseg,inst', ssc.CASES, ids=[c[0] for c in ssc.CASES])
def test_instance_matches_oracle(cid, nb, four, minseg, inst, oracle):
    _run(oracle, nb, four, minseg, inst)


def test_size_table_scan_matches_oracle(oracle):
    (cid, nb, four, minseg, inst) = ssc.SCAN
    _run(oracle, nb, four, minseg, inst, scan=True)


def test_counter_reset_and_argument():
    from pyshepseg_amd import _lib
    assert _lib.lib().shp_small_loop_instances(None, 0) != 0
    _instances(True)
    assert _instances(False) == [0, 0, 0, 0, 0]


def _same(got, sfx, wanted):
    wseg, wmx, whist = wanted
    assert int(got['max_seg_id' + sfx]) == wmx
    assert np.array_equal(got['seg' + sfx], wseg)
    assert np.array_equal(got['hist' + sfx], whist)


def test_mixed_batch_matches_oracle(oracle, tmp_path):
    """4- and 8-connected six-band jobs pending together on one walker stream: a launch whose jobs agree takes
    their instance, a launch whose jobs disagree the generic one; every launch is counted once"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    img, centres = ssw.image6()
    out = str(tmp_path / 'out.npz')
    env = dict(os.environ)
    for k in ('SHEPSEG_WALK_STREAMS', 'SHEPSEG_DFS_PER_WG', 'SHEPSEG_SMALL_BLOCKS', 'SHEPSEG_SMALL_MAX',
              'SHEPSEG_SHARED_STREAMS', 'SHEPSEG_SMALL_TIMING'):
        env.pop(k, None)
    env['SHEPSEG_WALK_STREAMS'] = '1'
    if wbc.ABNORMAL:
        pytest.fail('not started: child %s ended abnormally' % wbc.ABNORMAL[0])
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'small_spec_worker.py'), out, '8'], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        wbc.ABNORMAL.append('small_spec mixed (timeout)')
        pytest.fail('child timed out')
    if p.returncode < 0 or p.returncode in (134, 139):
        wbc.ABNORMAL.append('small_spec mixed (exit %d)' % p.returncode)
    assert p.returncode == 0, 'child exit %d:\n%s' % (p.returncode, p.stderr[-3000:])
    with np.load(out) as f:
        got = {k: f[k] for k in f.files}
    for (sfx, four) in (('4', True), ('8', False)):
        _same(got, sfx, seg_cases.oracle_tiled(oracle, img, centres, wbw.TILE, wbw.OVERLAP, wbw.MINSEG, wbw.MSD,
                                               None, four))
    l_launch, l_jobs = int(got['stats'][3]), int(got['stats'][4])
    inst = [int(v) for v in got['inst']]
    print('pass loop: %d launches of %d jobs; per instance (generic, 6/4, 6/8, 10/4, 10/8): %s'
          % (l_launch, l_jobs, inst))
    assert l_jobs == 2 * 24                                    # every tile of both runs ran one pass loop
    # every launch is counted under exactly one instance: the generic one (jobs that disagree) or a six-band one
    assert inst[ssc.GENERIC] + inst[ssc.B6_C4] + inst[ssc.B6_C8] == l_launch
    assert inst[ssc.B10_C4] == 0 and inst[ssc.B10_C8] == 0
    # All jobs are six-band and nothing asks for diagnostics, so a launch is generic only if its jobs disagree on
    # the connectivity: a generic launch IS a mixed batch.  With one walker stream the sixteen workers of the two
    # runs queue their jobs behind the launch that is out, and the next leader takes them all.
    assert inst[ssc.GENERIC] >= 1, 'no launch carried jobs of both connectivities'
    assert l_launch < l_jobs                                   # (batches formed at all)
