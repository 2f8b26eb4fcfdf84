"""CPU census of the rasters of tests/test_gpu_small_spec.py (tests/small_spec_cases.py): the oracle alone shows
that every case has passes in each range of pairs per source, that the merge step sees both its forms, and that the
size-table scan case has a pass above and passes below SMALL_BALANCED_MAX sources."""
import numpy as np
import pytest

import small_spec_cases as ssc


@pytest.mark.parametrize('cid,nb,four,minseg,inst', ssc.CASES, ids=[c[0] for c in ssc.CASES])
def test_passes_in_every_pair_range(cid, nb, four, minseg, inst, oracle):
    assert ssc.eliminated(oracle, nb, four, 2) == 0          # (targets start at 1: nothing below size 1)
    for (lo, hi) in ssc.pair_ranges(four, minseg):
        below, upto = ssc.eliminated(oracle, nb, four, lo), ssc.eliminated(oracle, nb, four, hi + 1)
        print('%s: targets %d..%d eliminate %d segments' % (cid, lo, hi, upto - below))
        assert upto > below, 'no merging pass with a target in %d..%d' % (lo, hi)
    # the merge step: a thread per source up to target 16, a wavefront per source above
    assert ssc.eliminated(oracle, nb, four, 17) > ssc.eliminated(oracle, nb, four, 2)
    assert ssc.eliminated(oracle, nb, four, minseg) > ssc.eliminated(oracle, nb, four, 17)


def test_instances_of_the_cases():
    """6 and 10 bands have instances of their own, 3 and 9 bands run the generic one"""
    want = {(6, True): ssc.B6_C4, (6, False): ssc.B6_C8, (10, True): ssc.B10_C4, (10, False): ssc.B10_C8}
    for (cid, nb, four, minseg, inst) in ssc.CASES + [ssc.SCAN]:
        assert inst == want.get((nb, four), ssc.GENERIC), cid


def test_scan_case_has_both_branches(oracle):
    (cid, nb, four, minseg, inst) = ssc.SCAN
    assert minseg > 256                                       # the per-size lists are off
    # after the single-pixel stage the first pass (target 2) has more sources than the balanced deal takes
    sizes = np.bincount(ssc.oracle_run(oracle, nb, four, 2, True)['segimg'].ravel())[1:]
    assert int((sizes == 2).sum()) > ssc.SMALL_BALANCED_MAX
    # from target 70 on fewer segments than that are below minSegmentSize at all: every later pass is balanced,
    # and such passes merge something
    sizes = np.bincount(ssc.oracle_run(oracle, nb, four, 70, True)['segimg'].ravel())[1:]
    assert 0 < int(((sizes > 0) & (sizes < minseg)).sum()) <= ssc.SMALL_BALANCED_MAX
    assert ssc.eliminated(oracle, nb, four, minseg, True) > ssc.eliminated(oracle, nb, four, 70, True)
