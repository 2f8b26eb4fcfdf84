"""The per-segment statistics kernels (csrc/segstats.h) at their run and patch edges: every case of
tests/stats_edge_cases.py through every entry it applies to -- calcPerSegmentStats (the sorts: k_seg_stats and
k_seg_stats_big), shp_segstats2d_dev with SHEPSEG_STATS_PATCH at '1', '0' and unset (k_stats_patch and what it leaves
to the sorts), shp_segstats2d_bands_dev with one, two and three bands (k_stats_patch_bands).  The sort-path cases are
1 x N rasters with scattered pixels: the 2-D entries leave nearly all of them to the sorts, which then run behind the
patch path's row filter at the same edges.  What each case reaches is counted on the host in
tests/test_stats_edge_cases_host.py.

Integer columns equal the oracle's and the numpy model's, dtype included; float columns have the oracle's bits; row 0
is zero; the words before and behind the columns keep their filler (asserted inside the entry helpers).  No tolerance
anywhere."""
import numpy as np
import pytest

import stats_edge_cases as sc

pytestmark = pytest.mark.gpu

_want = {}


def want(case, oracle):
    """per band: (oracle's integer columns, oracle's float columns, the model's integer columns), computed once"""
    if case.name not in _want:
        (seg, bands, nulls, S) = case.data()
        names = sc.int_names(case.pcs)
        out = []
        for (b, (ic, fc)) in enumerate(sc.expected(case, oracle)):
            model = sc.int_model(seg, bands[b], nulls[b], S, case.missing, case.pcs)
            mc = np.stack([model[k] for k in names])
            mc.flags.writeable = False
            out.append((ic, fc, mc))
        if seg.size > (1 << 20):
            return out
        _want[case.name] = out
    return _want[case.name]


def check(tag, got, expect, names):
    (ic, fc) = got
    (wic, wfc, mc) = expect
    assert ic.dtype == np.int64 and fc.dtype == np.float32, tag
    assert ic.shape == wic.shape and fc.shape == wfc.shape, tag
    assert (ic[:, 0] == 0).all() and (fc.view(np.uint32)[:, 0] == 0).all(), tag + ': row 0'
    for (k, name) in enumerate(names):
        bad = np.flatnonzero(ic[k] != wic[k])
        assert bad.size == 0, '%s: %s differs from the oracle in %d rows, first id %d: %d, expected %d' % (
            tag, name, bad.size, bad[0], ic[k][bad[0]], wic[k][bad[0]])
        assert np.array_equal(ic[k], mc[k]), '%s: %s differs from the numpy model' % (tag, name)
    for (k, name) in enumerate(('mean', 'stddev')):
        bad = np.flatnonzero(fc[k].view(np.uint32) != wfc[k].view(np.uint32))
        assert bad.size == 0, '%s: %s differs from the oracle in %d rows, first id %d: %r, expected %r' % (
            tag, name, bad.size, bad[0], fc[k][bad[0]], wfc[k][bad[0]])


@pytest.mark.parametrize('case', sc.CASES, ids=lambda c: c.name)
def test_stats_edge_case(case, oracle):
    (seg, bands, nulls, S) = case.data()
    expect = want(case, oracle)
    names = sc.int_names(case.pcs)
    sel = case.sel()
    for (b, null) in enumerate(nulls):
        check('%s flat band %d' % (case.name, b), sc.flat(seg, bands[b], sel, null, case.missing, S), expect[b], names)
    if 'patch' not in case.entries:
        return
    for knob in ('1', '0', None):
        for (b, null) in enumerate(nulls):
            got = sc.patch1(seg, bands[b], sel, null, case.missing, S, knob)
            check('%s patch1 knob=%r band %d' % (case.name, knob, b), got, expect[b], names)
    plans = [tuple(range(nb)) for nb in (1, 2, 3)] + [(2, 0), (1,)]
    if case.bands_extra:
        plans.append((0, 1, 2, 0))                      # four entries: both halves of the fill counter serve twice
    for knob in ('1', None):
        for plan in plans:
            if max(plan) >= len(nulls):
                continue
            got = sc.patchN(seg, [bands[b] for b in plan], sel, [nulls[b] for b in plan], case.missing, S, knob)
            for (k, b) in enumerate(plan):
                check('%s patchN knob=%r bands %r entry %d' % (case.name, knob, plan, k), got[k], expect[b], names)
