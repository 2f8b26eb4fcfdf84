"""CPU: what the GPU tests of the batched replay and pass loop (tests/test_gpu_walk_batch.py,
tests/test_gpu_walk_batch_uneven.py) rest on.  tests/walk_batch_cases.py counts, per tile window of the 'uneven'
raster, the components above the depth-first cut's cap (a replay job of ceil(n / SHEPSEG_DFS_PER_WG) workgroups
each) and the small segments the oracle eliminates; here the properties the GPU cases need are asserted, so that a
change of the raster that would turn them back into one-workgroup batches fails without a GPU.  The expected number
of replay jobs and the sum of their workgroups per (connectivity, per-wg) come from
walk_batch_cases.expected_replay."""
import pytest

import walk_batch_cases as wbc


@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
def test_uneven_raster_census(oracle, four):
    comps, elim = wbc.census(oracle, 'uneven', four)
    print('cut components per tile:', comps)
    print('small segments eliminated per tile:', elim)
    for per_wg in (1, 3, wbc.DFS_WAVES):
        print('per-wg %d: replay jobs %d, workgroups %d' % ((per_wg,) + wbc.expected_replay(comps, per_wg)))
    assert len(comps) == 24
    # one walker per workgroup: jobs of several sizes in one launch, one of them larger than DFS_WAVES
    one = wbc.job_blocks(comps, 1)
    assert len(set(one)) >= 4 and max(one) >= 8
    # the default: two-workgroup jobs among one-workgroup ones, and a tile whose worker skips the replay
    dflt = wbc.job_blocks(comps, wbc.DFS_WAVES)
    assert 2 in dflt and 1 in dflt and 0 in comps
    # every tile runs a pass loop
    assert min(elim) >= 1
    for per_wg in (1, 3, wbc.DFS_WAVES):
        jobs, blocks = wbc.expected_replay(comps, per_wg)
        assert jobs == sum(1 for n in comps if n > 0) and blocks >= jobs
    # three walkers per workgroup: a job whose last workgroup has idle walkers, and one of more than one workgroup
    assert any(n % 3 for n in comps if n > 3)
