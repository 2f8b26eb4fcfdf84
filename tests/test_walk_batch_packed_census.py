"""CPU: what tests/test_gpu_walk_batch_packed.py rests on.  tests/walk_batch_packed.py restates how a replay job is
sized by its work (csrc/clump.h dfs_job_blocks) and measures, per tile window of its raster, the components above
the depth-first cut's cap; here the properties the GPU cases need are asserted, so that a change of the raster or
of the rule that would turn the packed jobs back into a walker per component fails without a GPU."""
import os
import re

import pytest

import walk_batch_packed as wbp
from conftest import ROOT


def header_constant(name):
    """the text of a #define of pyshepseg_amd/csrc/clump.h"""
    with open(os.path.join(ROOT, 'pyshepseg_amd', 'csrc', 'clump.h')) as f:
        return re.search(r'^#define %s (.+?)\s*(?://.*)?$' % name, f.read(), flags=re.M).group(1)


def test_restated_constants_are_the_headers():
    assert float(header_constant('DFS_FILL')) == wbp.DFS_FILL
    assert header_constant('DFS_WAVES') == '%du' % wbp.DFS_WAVES
    assert header_constant('DFS_MAX_BLOCKS') == '%du' % wbp.DFS_MAX_BLOCKS
    assert header_constant('DFS_PACK_MIN') == '(2u * DFS_WAVES)' and wbp.DFS_PACK_MIN == 2 * wbp.DFS_WAVES


def test_rule_by_hand():
    """the benchmark tile of the rule's description (297 components, 7.54 Mpx, the largest 105 243 px), the floor,
    the clamp to a walker per component, and one workgroup at the least"""
    bench = [105243] + [(7540000 - 105243) // 296] * 296
    assert [wbp.packed_blocks(bench, f) for f in (1.0, 0.75, 0.5)] == [9, 12, 18]
    assert wbp.packed_blocks([20000] * 16) == 2 and wbp.packed_blocks([90000] + [10002] * 15) == 2
    assert wbp.packed_blocks([20000] * 17) == 3             # equal sizes: a walker each, as without the rule
    assert wbp.packed_blocks([10 ** 6] + [10002] * 16) == 1
    assert wbp.packed_blocks([10002] * 3000) == wbp.DFS_MAX_BLOCKS


@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
def test_packed_raster_census(oracle, four):
    sizes = wbp.census(oracle, four)
    assert len(sizes) == wbp.NTILES
    for s in sizes:
        print('%2d components, sum %7d, largest %6d, smallest %6d: %d workgroups packed, %d unpacked'
              % (len(s), sum(s), max(s), min(s), wbp.packed_blocks(s), wbp.unpacked_blocks(len(s))))
    packed = [s for s in sizes if wbp.packed_blocks(s) < wbp.unpacked_blocks(len(s))]
    # four tiles of at least 17 components of clearly unequal size, whose job is smaller than a walker per component
    assert len(packed) >= 4
    assert all(len(s) >= 17 and max(s) >= 3 * sorted(s)[len(s) // 2] for s in packed)
    # ... so much smaller that components are pulled from the job's counter
    assert all(wbp.packed_blocks(s) * wbp.DFS_WAVES < len(s) for s in packed)
    # a job of more than one workgroup among them: the interleaved first pass w * nblk + bid, then the counter
    assert any(wbp.packed_blocks(s) >= 2 for s in packed)
    # and a tile of 9 to 16 components, which keeps a walker per component
    assert any(9 <= len(s) <= wbp.DFS_PACK_MIN and wbp.packed_blocks(s) == 2 for s in sizes)
