"""The batch kernels beyond one-workgroup jobs (csrc/clump.h k_dfs_pool, csrc/elim_small.h k_small_loop, the
batcher of csrc/walkbatch.h): tiled runs of the 'uneven' raster of tests/walk_batch_worker.py, whose 24 tiles hold
0 to 9 components above the depth-first cut's cap (tests/test_walk_batch_census.py pins that on the CPU), under
knobs that make the jobs of one launch differ in workgroup count, change the pass loop's group size, bind the
residency budget, approach the job cap, and take the batcher out.  Every case compares labels, histogram and
maxSegId with the oracle exactly and the batcher's counters (shp_walk_batch_stats, shp_walk_batch_blocks) with the
CPU census: a replay job is a tile with n > 0 such components and has min(256, ceil(n / SHEPSEG_DFS_PER_WG))
workgroups, every tile runs one pass loop of SHEPSEG_SMALL_BLOCKS workgroups.  Where the workers share streams,
every job also books a count of one and a share of the launch's time under the replay's and the pass loop's
profile ids, summed over the worker contexts as bench.py sums them.

What a case pins in the kernels:
  dfs_per_wg_1   jobs of 3, 4, 5, 7 and 9 workgroups in one launch: the prefix walk over DfsBatch::pre, bid and nblk
                 of a job that does not start at workgroup 0, the first-pass index w * nblk + bid and the snapshot
                 slot bid * nwalk + w with nwalk = 1
  dfs_per_wg_3   the same with nwalk = 3: slots bid * 3 + w, walkers beyond a job's components idle
  dfs_default    two-workgroup jobs among one-workgroup ones at eight walkers
  small_blocks_13, small_blocks_1   groups of 13 and of 1 workgroup: blockIdx.x / nblk, groups that start on
                 rotating XCDs, the per-group xcd_n count of the two-level barrier
  small_max_3    the residency budget binds a batch
  workers_24     batches near the cap of DFS_MAX_JOBS records by value in the kernel arguments
  both_at_once   a 4-connected and an 8-connected run share launches: `four` read from the job's own record
  unshared, one_worker   every launch carries one job
The library reads its knobs once per process, so every setting runs in a fresh child, one at a time, 120 s at the
most; after a child that ended abnormally or timed out none is started."""
import numpy as np
import pytest

import seg_cases
import walk_batch_cases as wbc
import walk_batch_worker as wbw

pytestmark = pytest.mark.gpu

RASTER = 'uneven'
NTILES = 24
WS1 = {'SHEPSEG_WALK_STREAMS': '1'}

# (id, environment, connectivity, workers)
CASES = [
    ('dfs_per_wg_1', dict(WS1, SHEPSEG_DFS_PER_WG='1'), 'four', 8),
    ('dfs_per_wg_1', dict(WS1, SHEPSEG_DFS_PER_WG='1'), 'eight', 8),
    ('dfs_per_wg_3', dict(WS1, SHEPSEG_DFS_PER_WG='3'), 'four', 8),
    ('dfs_per_wg_3', dict(WS1, SHEPSEG_DFS_PER_WG='3'), 'eight', 8),
    ('dfs_default', dict(WS1), 'four', 8),
    ('two_streams_per_wg_1', {'SHEPSEG_WALK_STREAMS': '2', 'SHEPSEG_DFS_PER_WG': '1'}, 'eight', 8),
    ('small_blocks_13', dict(WS1, SHEPSEG_SMALL_BLOCKS='13'), 'four', 8),
    ('small_blocks_1', dict(WS1, SHEPSEG_SMALL_BLOCKS='1'), 'four', 8),
    ('small_max_3', dict(WS1, SHEPSEG_SMALL_MAX='3'), 'four', 8),
    ('workers_24', dict(WS1, SHEPSEG_DFS_PER_WG='1'), 'four', 24),
    ('unshared', {'SHEPSEG_SHARED_STREAMS': '0'}, 'four', 8),
    ('one_worker', {}, 'four', 1),
    ('both_at_once', dict(WS1, SHEPSEG_DFS_PER_WG='1'), 'both', 8),
]


@pytest.fixture(scope='module')
def want(oracle):
    img, centres = wbw.image_uneven()
    cache = {}

    def get(four):
        if four not in cache:
            cache[four] = seg_cases.oracle_tiled(oracle, img, centres, wbw.TILE, wbw.OVERLAP, wbw.MINSEG, wbw.MSD,
                                                 None, four)
        return cache[four]
    return get


def test_expected_mosaics(want):
    """the case is what its description says: the oracle's segment counts"""
    assert want(True)[1] == 365 and want(False)[1] == 165


def _same(got, sfx, wanted):
    wseg, wmx, whist = wanted
    assert int(got['max_seg_id' + sfx]) == wmx
    assert np.array_equal(got['seg' + sfx], wseg)
    assert np.array_equal(got['hist' + sfx], whist)


@pytest.mark.parametrize('setting,env,conn,workers', CASES, ids=['%s-%s' % (c[0], c[2]) for c in CASES])
def test_uneven_tiles_match_oracle_and_census(setting, env, conn, workers, want, oracle, tmp_path):
    name = '%s/%s' % (setting, conn)
    got = wbc.run_child(name, env, {'four': '1', 'eight': '0', 'both': 'both'}[conn], workers, RASTER,
                        str(tmp_path / 'out.npz'))
    r_launch, r_jobs, r_big, l_launch, l_jobs, l_big = [int(v) for v in got['stats']]
    r_blocks, r_most, l_blocks, l_most = [int(v) for v in got['blocks']]
    prof_cnt, prof_ms = [int(v) for v in got['prof_cnt']], [float(v) for v in got['prof_ms']]
    print('%s: replay launches %d jobs %d largest %d workgroups %d most %d; pass loop launches %d jobs %d largest %d '
          'workgroups %d most %d; profile counts %d / %d, ms %.3f / %.3f'
          % (name, r_launch, r_jobs, r_big, r_blocks, r_most, l_launch, l_jobs, l_big, l_blocks, l_most,
             prof_cnt[0], prof_cnt[1], prof_ms[0], prof_ms[1]))
    if conn == 'both':
        _same(got, '4', want(True))
        _same(got, '8', want(False))
    else:
        _same(got, '', want(conn == 'four'))

    # the counters against the census
    per_wg = int(env.get('SHEPSEG_DFS_PER_WG', wbc.DFS_WAVES))
    small_blocks = int(env.get('SHEPSEG_SMALL_BLOCKS', wbc.SMALL_BLOCKS))
    conns = [True, False] if conn == 'both' else [conn == 'four']
    comps = [wbc.census(oracle, RASTER, f)[0] for f in conns]
    job_blocks = sum((wbc.job_blocks(c, per_wg) for c in comps), [])
    want_jobs = sum(wbc.expected_replay(c, per_wg)[0] for c in comps)
    want_blocks = sum(wbc.expected_replay(c, per_wg)[1] for c in comps)
    assert (r_jobs, r_blocks) == (want_jobs, want_blocks)
    assert (l_jobs, l_blocks) == (NTILES * len(conns), small_blocks * NTILES * len(conns))
    assert 1 <= r_launch <= r_jobs and 1 <= l_launch <= l_jobs
    assert 1 <= r_big <= wbc.DFS_MAX_JOBS and max(job_blocks) <= r_most <= r_blocks
    assert l_most == l_big * small_blocks           # equal groups: the largest batch is the largest launch

    batched = setting not in ('unshared', 'one_worker')
    if setting != 'unshared':
        # stream-sharing workers: every member of a batch books one launch and a share of its time
        assert prof_cnt == [r_jobs, l_jobs]
        assert prof_ms[0] > 0.0 and prof_ms[1] > 0.0
    if not batched:
        assert (r_launch, l_launch) == (r_jobs, l_jobs)
    if setting == 'unshared':
        assert (r_big, l_big) == (1, 1)
    if setting in ('dfs_per_wg_1', 'dfs_per_wg_3'):
        # with one walker stream the pending jobs accumulate behind the launch that is out.  The launch of the
        # most workgroups carries at most r_big jobs: a real batch of jobs of more than one workgroup ...
        assert r_big >= 2 and r_most >= r_big + 2
        # ... by the census alone: more workgroups than any one job has, and than all one-workgroup jobs together
        assert r_most > max(max(job_blocks), sum(1 for b in job_blocks if b == 1))
    if setting == 'small_blocks_13':
        assert l_big >= 2
    if setting == 'small_max_3':
        assert l_big in (2, 3) and l_launch >= NTILES // 3
    if setting == 'workers_24':
        # (whether a launch reaches the cap of DFS_MAX_JOBS records depends on timing: printed, not asserted)
        print('%s: largest replay batch %d of at most %d' % (name, r_big, wbc.DFS_MAX_JOBS))
