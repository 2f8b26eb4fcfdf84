"""What tests/single_tail_cases.py claims about its tiles, asserted on the CPU: the reference's loop in plain Python
(single_tail_cases.model) against the oracle's single-pixel stage, and per case the pass and candidate counts that
make k_single_tail take each of its branches (csrc/elim_single.h)."""
import numpy as np
import pytest

import single_tail_cases as stc

_runs = {}


def run(oracle, name):
    if name not in _runs:
        img, cen, nullv, four = stc.build(name)
        cl = oracle.kmeans_assign(img, cen, nullv).astype(np.int32)
        seg, nxt = oracle.clump(cl, 0, four, 1)
        sizes0 = np.bincount(seg.ravel())
        mseg = seg.copy()
        m = stc.model(img, mseg, four)
        oseg = seg.copy()
        osz = oracle.make_seg_size(oseg)
        total = oracle.eliminate_single_pixels(img, oseg, osz, 1, nxt - 1, four)
        _runs[name] = dict(m=m, mseg=mseg, oseg=oseg, total=total, n=seg.size, nnull=int((cl == 0).sum()),
                           singles0=int((sizes0[seg] == 1).sum()), sizes0=sizes0)
    return _runs[name]


@pytest.mark.parametrize('name', sorted(stc.CASES))
def test_model_is_the_oracles_stage(oracle, name):
    r = run(oracle, name)
    # (the oracle's stage ends with the reference's relabelSegments: ids in order, 0 kept for null)
    ids, rank = np.unique(r['mseg'], return_inverse=True)
    rank = rank.reshape(r['mseg'].shape) + (0 if ids[0] == 0 else 1)
    assert np.array_equal(rank, r['oseg']) and r['m']['total'] == r['total']
    # every single pixel merges in the end, and the later passes (the tail's) do part of it
    assert r['total'] == r['singles0'] and len(r['m']['passes']) >= 2
    # the small-segment stage has nothing to do: the GPU cases compare the single-pixel stage's labels
    left = np.bincount(r['oseg'].ravel())
    assert left[1:][left[1:] > 0].min() >= stc.MINSEG


def test_blocks_peel_a_ring_per_pass(oracle):
    for name, k in (('k3', 3), ('k8', 8), ('k40', 40), ('k40_eight', 40), ('k36', 36), ('k36_u32', 36)):
        p = run(oracle, name)['m']['passes']
        assert len(p) == (k + 1) // 2, name
        assert [c for c, _ in p] == [(k - 2 * t) ** 2 for t in range(len(p))], name
    assert len(run(oracle, 'k40')['m']['passes']) == 20


def test_list_lengths_around_one_round(oracle):
    # the tail's first list is what the first pass left: above 1024 a thread takes several candidates, from 1024 down one
    for name in ('k36', 'k36_u32'):
        p = run(oracle, name)['m']['passes']
        assert p[1][0] == 34 * 34 > stc.TAIL_THREADS and p[2][0] == 32 * 32 == stc.TAIL_THREADS
    p = run(oracle, 'k40')['m']['passes']
    assert [c for c, _ in p[1:5]] == [1444, 1296, 1156, 1024]
    assert run(oracle, 'k3')['m']['passes'][1][0] == 1


def test_patterned_all_over_does_not_compact(oracle):
    r = run(oracle, 'all_over')
    p = r['m']['passes']
    assert 2 * p[1][0] > r['n'] and len(p) >= 30
    assert r['singles0'] == r['n'] - 3


def test_nulls_ties_and_wraps(oracle):
    r = run(oracle, 'nulls')
    assert r['nnull'] == 12 and r['m']['target0']
    r = run(oracle, 'one_null')
    assert r['nnull'] == 1          # segment 0 is a one-pixel segment: the GPU path scans every pixel instead of the list
    assert not r['m']['target0']
    assert run(oracle, 'ties')['m']['tie']         # without noise: two segments at the same distance, the first wins
    for name in ('corner', 'k36_u32', 'flat_i32', 'wrap_u32'):
        assert run(oracle, name)['m']['negative'], name
    for name in ('k40', 'k8', 'k40_eight'):
        assert not run(oracle, name)['m']['negative'], name


def test_cases_cover_bands_types_and_connectivities():
    c = stc.CASES.values()
    assert {v[3] for v in c} == {1, 6, 8, 9}
    assert {v[4] for v in c} == set(stc.LEVELS)
    assert {v[5] for v in c} == {True, False}
    assert all(v[0] <= 128 and v[1] <= 128 for v in c)
