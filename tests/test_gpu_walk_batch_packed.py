"""Replay jobs sized by their work (csrc/clump.h dfs_job_blocks, k_big_order's mirror words, k_dfs_pool's pull from
the job's counter): tiled runs of the 'packed' raster of tests/walk_batch_packed.py, four of whose five tiles hold
18 to 20 components above the depth-first cut's cap, one of them several times the others, so that their jobs get
fewer walkers than components (tests/test_walk_batch_packed_census.py pins that on the CPU).  Every case compares
labels, histogram and maxSegId with the oracle exactly, and the replay's job count and workgroup sum
(shp_walk_batch_blocks) with the restated rule on the CPU census.

What a case pins:
  one_stream     (both connectivities) one walker stream, so that pending jobs gather behind the launch that is
                 out: a packed job shares a launch with another job, and its walkers pull components from the
                 job's counter inside a batch
  default        the default stream pools
  unshared       SHEPSEG_SHARED_STREAMS=0: the direct launch of a packed job
  per_wg_8       SHEPSEG_DFS_PER_WG=8 set explicitly switches the packing off: ceil(n / 8) workgroups per job
The library reads its knobs once per process, so every setting runs in a fresh child
(walk_batch_cases.run_child), one at a time; after a child that ended abnormally none is started."""
import os

import numpy as np
import pytest

import seg_cases
import walk_batch_cases as wbc
import walk_batch_packed as wbp
import walk_batch_worker as wbw

pytestmark = pytest.mark.gpu

WORKERS = 8
# (id, environment, connectivity)
CASES = [
    ('one_stream', {'SHEPSEG_WALK_STREAMS': '1'}, 'four'),
    ('one_stream', {'SHEPSEG_WALK_STREAMS': '1'}, 'eight'),
    ('default', {}, 'four'),
    ('unshared', {'SHEPSEG_SHARED_STREAMS': '0'}, 'four'),
    ('per_wg_8', {'SHEPSEG_WALK_STREAMS': '1', 'SHEPSEG_DFS_PER_WG': '8'}, 'four'),
]


@pytest.fixture(scope='module')
def want(oracle):
    img, centres = wbp.image_packed()
    cache = {}

    def get(four):
        if four not in cache:
            cache[four] = seg_cases.oracle_tiled(oracle, img, centres, wbp.TILE, wbp.OVERLAP, wbw.MINSEG, wbw.MSD,
                                                 None, four)
        return cache[four]
    return get


@pytest.fixture()
def packed_worker(monkeypatch):
    """walk_batch_cases.run_child starts tests/walk_batch_packed.py: the shared worker on this raster and tiling"""
    monkeypatch.setattr(wbc, 'WORKER', os.path.join(wbc.ROOT, 'tests', 'walk_batch_packed.py'))


@pytest.mark.parametrize('setting,env,conn', CASES, ids=['%s-%s' % (c[0], c[2]) for c in CASES])
def test_packed_tiles_match_oracle_and_rule(setting, env, conn, want, oracle, tmp_path, packed_worker):
    four = conn == 'four'
    name = '%s/%s' % (setting, conn)
    got = wbc.run_child(name, env, '1' if four else '0', WORKERS, 'packed', str(tmp_path / 'out.npz'))
    r_launch, r_jobs, r_big = [int(v) for v in got['stats'][:3]]
    r_blocks, r_most = [int(v) for v in got['blocks'][:2]]
    print('%s: replay launches %d jobs %d largest batch %d workgroups %d most %d'
          % (name, r_launch, r_jobs, r_big, r_blocks, r_most))
    wseg, wmx, whist = want(four)
    assert int(got['max_seg_id']) == wmx
    assert np.array_equal(got['seg'], wseg)
    assert np.array_equal(got['hist'], whist)

    sizes = wbp.census(oracle, four)
    if setting == 'per_wg_8':
        blocks = [wbp.unpacked_blocks(len(s), 8) for s in sizes]
        assert blocks == [-(-len(s) // 8) for s in sizes]
    else:
        blocks = [wbp.packed_blocks(s) for s in sizes]
        # (the census test's conditions, where they matter: fewer walkers than components in four jobs)
        assert sum(1 for (b, s) in zip(blocks, sizes) if b * wbp.DFS_WAVES < len(s)) >= 4
    print('%s: workgroups per job by the rule %s' % (name, blocks))
    assert (r_jobs, r_blocks) == (len(sizes), sum(blocks))
    assert 1 <= r_launch <= r_jobs and max(blocks) <= r_most <= r_blocks
    if setting == 'unshared':
        assert (r_launch, r_big) == (r_jobs, 1) and r_most == max(blocks)
    if setting == 'one_stream':
        # some launch carried more workgroups than the largest job has: a batch.  Every job but the last tile's
        # is a packed one, so a batch of two jobs holds one
        assert r_big >= 2 and r_most > max(blocks)
