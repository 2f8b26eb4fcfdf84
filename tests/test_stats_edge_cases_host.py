"""CPU: the cases of tests/stats_edge_cases.py reach what their names say -- counted from the constants parsed out of
csrc/segstats.h -- the numpy model of the integer statistics agrees with the oracle on every one of them and on
examples worked by hand, and the high-precision bound on the float columns holds for the oracle itself."""
import numpy as np
import pytest

import stats_edge_cases as sc

CASE = sc.BY_NAME


def band0(name):
    (seg, bands, nulls, S) = CASE[name].data()
    return seg, bands[0], nulls[0], S


def flat_census(name):
    (seg, band, null, S) = band0(name)
    return sc.sort_census(sc.flat_keys(seg, band, null, S), S)


def patches(name, b=0):
    (seg, bands, nulls, S) = CASE[name].data()
    return sc.patch_census(seg, bands[b], nulls[b], S)


def label(p, i):
    """the entry of label i in a patch record"""
    (k,) = np.flatnonzero(p['ids'] == i)
    return {key: p[key][k] for key in ('pix', 'valid', 'complete1', 'completeN')}


def test_constants_are_the_header():
    assert sc.PATCH == 2048 and sc.PATCH % 256 == 0
    assert sc.SLOTS & (sc.SLOTS - 1) == 0 and sc.SLOTS == 1 << (32 - sc.HASH_SHIFT)
    assert sc.MAXDIST < sc.SLOTS < sc.PATCH and sc.MAXRUN == 64 and sc.STAGE < sc.BIG and sc.STAGE % 64 == 0
    assert sc.BIG_WAVES == 2048
    if (sc.STAGE, sc.BIG, sc.MAXDIST, sc.SLOTS) == (3072, 4096, 704, 1024):
        assert sc.A1_SIZES == (1, 2, 63, 64, 65, 3071, 3072, 3073, 4095, 4096, 4097, 4159, 4160, 4161, 8192, 8193)
        assert sc.B4_COUNTS == (703, 704, 705, 1024, 1025, 2048)
    assert int(sc.home_slot([1])[0]) == (2654435761 >> 22) and int(sc.home_slot([0])[0]) == 0
    assert int(sc.home_slot([3])[0]) == ((3 * 2654435761) % (1 << 32)) >> 22


def test_percentile_scan():
    pairs = sc.percentile_float_pairs(1, 4200)
    assert len(pairs) == 586
    assert {(25, 28), (25, 56), (50, 14), (50, 28), (50, 56), (100, 7)} <= set(pairs)
    assert [q for q in pairs if q[0] <= 64] == [(25, 28), (25, 56), (50, 14), (50, 28), (50, 56)]
    for (n, p) in pairs:                                         # the float product lands ABOVE the integer
        assert sc.percentile_index(n, p) == -((-n * p) // 100)
    assert sc.percentile_index(25, 28) == 7 and sc.percentile_index(7, 0) == 6 and sc.percentile_index(7, 100) == 6
    big = sc.percentile_float_pairs(sc.BIG + 1, 3 * sc.BIG + 1)
    assert len(big) > 0
    (sizes, pcs, chosen) = sc.a8_plan()
    assert set(q for q in pairs if q[0] <= sc.MAXRUN) <= set(chosen) and (100, 7) in chosen
    assert sum(1 for (n, _p) in chosen if sc.MAXRUN < n <= sc.BIG) >= 5 and sum(1 for (n, _p) in chosen if n > sc.BIG) == 3
    assert {0, 1, 50, 99, 100} <= set(pcs) and {p for (_n, p) in chosen} <= set(pcs)
    (seg, band, null, S) = band0('A8-percentiles')
    cen = sc.sort_census(sc.flat_keys(seg, band, null, S), S)
    ids = CASE['A8-percentiles'].info['ids']
    assert all(cen['cnt'][ids[n]] == n for n in sizes)
    model = sc.int_model(seg, band, null, S, pcs=pcs)
    for (n, p) in chosen:                                        # values 0 .. n - 1: the column shows the index
        assert model['p%d' % p][ids[n]] == -((-n * p) // 100) == sc.percentile_index(n, p)


def test_model_by_hand():
    seg = np.array([[1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3, 0, 9]], dtype=np.uint32)
    band = np.array([[5, 3, 5, 3, 9, 4, 4, 7, 7, 0, 0, 6, 6]], dtype=np.uint16)
    m = sc.int_model(seg, band, 0, 4, missing=-5, pcs=(0, 20, 21, 100))
    #                 row 0  1: 3 3 5 5 9   2: 4 4 7 7   3: all nodata   4: no pixels (9 is above S)
    assert m['n'].tolist() == [0, 5, 4, 0, 0]
    assert m['mn'].tolist() == [0, 3, 4, -5, -5] and m['mx'].tolist() == [0, 9, 7, -5, -5]
    assert m['mode'].tolist() == [0, 3, 4, -5, -5]               # ties: the smallest value
    assert m['med'].tolist() == [0, 5, 4, -5, -5]                # ceil(2.5) - 1 = 2 -> 5; ceil(2.0) - 1 = 1 -> 4
    assert m['p0'].tolist() == [0, 9, 7, -5, -5]                 # p = 0: the last element
    assert m['p20'].tolist() == [0, 3, 4, -5, -5]                # ceil(1.0) - 1 = 0; ceil(0.8) - 1 = 0
    assert m['p21'].tolist() == [0, 3, 4, -5, -5]                # ceil(1.05) - 1 = 1 -> 3
    assert m['p100'].tolist() == [0, 9, 7, -5, -5]
    mean = np.array([0, 5, 5.5, -5, -5], dtype=np.float32)
    sd = np.sqrt(np.array([0, 24 / 5, 9 / 4, 25, 25], dtype=np.float64)).astype(np.float32)
    sd[3:] = -5
    assert sc.float_violations(seg, band, 0, 4, -5, mean, sd) == ''
    assert 'id 2: mean' in sc.float_violations(seg, band, 0, 4, -5, np.nextafter(mean, np.float32(9)), sd)
    worse = sd.copy()
    worse[1] = sd[1] * np.float32(1 + 6 * 2.0 ** -24)            # D = 3: six roundings on the variance are the limit
    assert 'id 1: stddev' in sc.float_violations(seg, band, 0, 4, -5, mean, worse)
    sd[4] = 0
    assert 'without valid pixels' in sc.float_violations(seg, band, 0, 4, -5, mean, sd)


def test_census_a1_to_a4():
    for name in ('A1-few-levels', 'A1-all-distinct'):
        cen = flat_census(name)
        ids = CASE[name].info['ids']
        assert [int(cen['cnt'][ids[n]]) for n in sc.A1_SIZES] == list(sc.A1_SIZES)
        assert len({i // 64 for i in ids.values()}) == len(sc.A1_SIZES)              # a wavefront of ids each
        assert sorted(cen['big'].tolist()) == sorted(ids[n] for n in sc.A1_SIZES if n > sc.BIG)
        assert cen['staged'].any() and not cen['staged'].all()
        (seg, band, null, S) = band0(name)
        sizes = {}
        for n in sc.A1_SIZES:
            v = band[(seg == ids[n]) & (band != null)]
            sizes[n] = len(np.unique(v))
            assert v.size == n
        assert all(d == n for (n, d) in sizes.items()) if name.endswith('distinct') else max(sizes.values()) <= 8
    cen = flat_census('A2-stage-limit')
    assert cen['span'][1] == sc.STAGE and cen['staged'][1]
    assert cen['span'][2] == sc.STAGE + 1 and not cen['staged'][2]
    assert cen['big'].tolist() == [200] and not cen['staged'][3] and (cen['cnt'][192:256] <= 6).sum() == 63
    info = CASE['A2-stage-limit'].info
    (seg, band, null, S) = band0('A2-stage-limit')
    assert all((seg == i).sum() == 0 for i in info['empty'])
    assert all((seg == i).sum() > 0 and (band[seg == i] == null).all() for i in info['allnull'])
    assert cen['staged'][4] and S % 64 != 63
    full = flat_census('A3-first-wave-unstaged')
    bare = flat_census('A3-first-wave-staged')
    assert full['cnt'][0] > sc.STAGE and not full['staged'][0] and len(full['staged']) == 1
    assert bare['cnt'][0] == 0 and bare['staged'][0] and np.array_equal(full['cnt'][1:], bare['cnt'][1:])
    for S in (62, 63, 64, 254, 255, 256):
        (seg, band, null, S_) = band0('A4-S%d' % S)
        assert S_ == S and (seg > S).sum() > 0 and (seg == S).sum() > 64
        assert len(flat_census('A4-S%d' % S)['span']) == S // 64 + 1


def test_census_a5_to_a9():
    segs = sc.a5_segments()
    cen = flat_census('A5-run-structure')
    ids = CASE['A5-run-structure'].info['ids']
    assert sorted(cen['big'].tolist()) == sorted(ids.values())
    (seg, band, null, S) = band0('A5-run-structure')
    for (name, a) in segs.items():
        got = np.sort(band[(seg == ids[name]) & (band != null)].astype(np.int64))
        assert np.array_equal(got, a), name
    heads = lambda a: np.flatnonzero(np.diff(a)) + 1              # where a new run begins
    assert (heads(segs['lane0']) % 64 == 0).all()
    assert set((heads(segs['runs63']) % 64).tolist()) == set(range(64)) == set((heads(segs['runs65']) % 64).tolist())
    c63 = segs['close63']
    run = np.flatnonzero(c63 == 10)
    assert run[0] % 64 != 0 and run[-1] % 64 == 63 and run.size > 128
    assert len(np.unique(segs['equal-big+1'])) == 1 and segs['equal-big+1'].size == sc.BIG + 1
    assert len(np.unique(segs['equal-2big'])) == 1 and segs['equal-2big'].size == 2 * sc.BIG
    assert len(np.unique(segs['distinct'])) == segs['distinct'].size
    for (name, where) in (('tie-two-longest', (0, 1)), ('longest-first', (0,)), ('longest-last', (-1,)), ('tie-last', (0, -1))):
        (u, c) = np.unique(segs[name], return_counts=True)
        assert sorted(np.flatnonzero(c == c.max()).tolist()) == sorted(w % len(u) for w in where), name
    for dt in ('uint8', 'int16', 'int32', 'uint32'):
        for (e, end) in enumerate(('min', 'max')):
            name = 'A6-%s-null-%s' % (dt, end)
            (seg, band, null, S) = band0(name)
            (lo, hi) = sc.LIMITS[dt]
            assert band.dtype == np.dtype(dt) and null == (lo, hi)[e]
            cen = flat_census(name)
            assert cen['big'].tolist() == [2] and cen['cnt'][1] == 40 and cen['cnt'][3] == 0
            for i in (1, 2):
                v = band[(seg == i) & (band != null)].astype(np.int64)
                assert v.min() == (lo + 1 if e == 0 else lo) and v.max() == (hi if e == 0 else hi - 1)
            assert (band[seg == 4] == (hi, lo)[e]).all()
    cen = flat_census('A7-second-trip')
    assert len(cen['big']) == sc.BIG_WAVES + 1 and (cen['cnt'][1:] == sc.BIG + 1).all()
    for m in (-9999, 7, -1):
        case = CASE['A9-missing%d' % m]
        (seg, band, null, S) = band0(case.name)
        assert case.missing == m and (seg > S).any() and (seg == 0).any()
        assert all((seg == i).sum() == 0 for i in case.info['empty'])
        assert all((seg == i).sum() > 0 and (band[seg == i] == null).all() for i in case.info['allnull'])


def test_census_b1_to_b3():
    for shape in sc.B1_SHAPES:
        (seg, bands, nulls, S) = CASE['B1-%dx%d' % shape].data()
        assert seg.shape == shape and len(set(nulls)) == 3
        valid = [((bands[b] != nulls[b]) & (seg != 0)).sum() for b in range(3)]
        assert shape == (1, 1) or len(set(valid)) > 1                               # the valid counts differ per band
        if shape[0] > 1:
            assert (seg[-1] == S).all()
        if shape[1] > 1:
            assert (seg[:, -1] == S).all()
        (ps, _f1, _fN) = patches('B1-%dx%d' % shape)
        assert len(ps) == -(-shape[0] // sc.PH) * -(-shape[1] // sc.PW)
    ((p,), f1, fN) = patches('B1-32x64')                # the label over the last row and column: too long for a patch
    assert fN.sum() == 1 and fN[-1] and label(p, 65)['pix'] == sc.PH + sc.PW - 1 and p['completeN'].sum() == 64
    (ps, f1, fN) = patches('B2-completeness')
    want = {1: (64, 64, True, True), 2: (65, 65, False, False), 3: (65, 64, True, False), 4: (12, 0, True, True)}
    for (i, w) in want.items():
        got = label(ps[0], i)
        assert (got['pix'], got['valid'], got['complete1'], got['completeN']) == w, i
    for (k, i, w) in ((1, 5, (sc.PATCH, 64, True, False)), (2, 6, (sc.PATCH, 65, False, False)), (3, 7, (sc.PATCH, 0, True, False))):
        got = label(ps[k], i)
        assert ps[k]['ndist'] == 1 and (got['pix'], got['valid'], got['complete1'], got['completeN']) == w, i
    assert f1[[1, 2, 3, 4, 5, 6, 7]].tolist() == [False, True, False, False, False, True, False]
    assert fN[[1, 2, 3, 4, 5, 6, 7]].tolist() == [False, True, True, False, True, True, True]
    assert ps[0]['complete1'].sum() > 10 and ps[4]['left1'] == 0                   # ordinary labels beside them
    # the other bands see other valid counts of the same labels
    assert label(patches('B2-completeness', 1)[0][1], 5)['valid'] == 63
    assert label(patches('B2-completeness', 2)[0][3], 7)['valid'] == 1
    (ps, f1, fN) = patches('B3-split-labels')
    seg = CASE['B3-split-labels'].data()[0]
    assert len(ps) == 4
    share = lambda i: sorted(int(label(p, i)['pix']) for p in ps if i in p['ids'])
    assert share(1) == [1, 63] and share(2) == [1, 63] and share(3) == [1, 1, 1, 61]
    assert {seg[5, 1], seg[5, sc.PW]} == {1} and seg[sc.PH, sc.PW + 36] == 2 and seg[sc.PH - 1, sc.PW + 36] == 2
    assert f1[[1, 2, 3]].all() and fN[[1, 2, 3]].all() and not f1[4:].all()


def test_census_b4_to_b6():
    for D in sc.B4_COUNTS:
        (ps, f1, fN) = patches('B4-%d-labels' % D)
        (p, q) = ps
        assert p['ndist'] == D and p['crowded'] == (D > sc.MAXDIST)
        assert q['ndist'] == 64 and not q['crowded'] and q['complete1'].all() and q['completeN'].all()
        if D <= sc.MAXDIST:
            assert p['complete1'].all() and p['completeN'].all() and p['left1'] == 0
            assert p['valid'].sum() == sc.PATCH                                         # every pixel valid in band 0
        else:
            assert not p['complete1'].any() and p['left1'] == sc.PATCH == p['leftN']
            assert f1[1:D + 1].all() and not f1[D + 1:].any()
        assert p['noslot_labels'] == max(0, D - sc.SLOTS) and (p['noslot_pixels'] > 0) == (D > sc.SLOTS)
        if D == sc.MAXDIST:
            assert p['words1'] == sc.PATCH + sc.MAXDIST == p['wordsN']                   # runs[] to its last word
    (ps, f1, fN) = patches('B5-collisions')
    info = CASE['B5-collisions'].info
    assert len(set(sc.home_slot(info['crowd']).tolist())) == 1 and len(info['crowd']) == 40
    assert set(info['crowd']) <= set(ps[0]['ids'].tolist()) and ps[0]['chain'] >= 39 and not ps[0]['crowded']
    assert sc.home_slot(info['tail']).tolist() == [sc.SLOTS - 1] * 6 + [sc.SLOTS - 2] * 2
    assert set(info['tail']) <= set(ps[1]['ids'].tolist()) and ps[1]['wrapped'] and ps[1]['chain'] >= 5
    (seg, bands, nulls, S) = CASE['B5-collisions'].data()
    assert S > 40000 and len(np.unique(seg)) < 200                                 # most rows are the prefill's
    for dt in ('uint8', 'int16', 'uint16', 'int32', 'uint32'):
        case = CASE['B6-rank-%s' % dt]
        (seg, bands, nulls, S) = case.data()
        (lo, hi) = sc.LIMITS[dt]
        assert nulls == [hi, lo, lo + 5]
        ids = case.info['ids']
        for b in range(3):
            ((p,), _f1, _fN) = sc.patch_census(seg, bands[b], nulls[b], S)
            assert p['complete1'].all() and p['completeN'].all()
            assert [int(label(p, ids['run%d' % n])['valid']) for n in sc.B6_RUNS] == list(sc.B6_RUNS)
            eq = bands[b][seg == ids['equal']]
            assert eq.size == sc.MAXRUN and len(np.unique(eq)) == 1
            de = bands[b][seg == ids['descending']].astype(np.int64)
            assert de.size == sc.MAXRUN and (np.diff(de) < 0).all()
            ex = bands[b][seg == ids['extremes']].astype(np.int64)
            ex = ex[ex != nulls[b]]
            assert ex.size == sc.MAXRUN - 1 and {int(ex.min()), int(ex.max())} == {lo, hi} - {nulls[b]} | \
                {lo + 1 if nulls[b] == lo else lo, hi - 1 if nulls[b] == hi else hi}
    assert sc.B6_RUNS == (1, 7, 8, 9, 15, 16, 17, 63, 64)


def test_census_b7_b8():
    case = CASE['B7-both-paths']
    (seg, bands, nulls, S) = case.data()
    (ps, f1, fN) = patches('B7-both-paths')
    assert (seg == 1).sum() == sc.BIG + 1 and f1[1] and fN[1]
    strad = case.info['straddlers']
    assert f1[strad].all() and len(strad) > 60 and all((seg == i).sum() == 2 for i in strad)
    assert np.array_equal(f1, fN)
    # ids 2 .. 2 * len(strad) + 1: flagged and unflagged take turns inside the first two wavefronts of ids
    turn = f1[2:2 * len(strad) + 2]
    assert turn[0::2].all() and not turn[1::2].any() and 2 * len(strad) + 2 > 64
    assert sum(int(p['complete1'].sum()) for p in ps) > 200
    cen = sc.sort_census(sc.left_keys(seg, bands[0], nulls[0], S, f1, True), S)
    assert cen['big'].tolist() == [1]                                              # the wavefront path, band 0
    cen1 = sc.sort_census(sc.left_keys(seg, bands[1], nulls[1], S, fN, False), S)
    assert cen1['big'].size == 0 and 0 < cen1['cnt'][0] and cen1['cnt'][1] > sc.STAGE   # ... and a thread's, band 1
    (ps, f1, fN) = patches('B7-nothing-left')
    assert not f1.any() and not fN.any() and all(p['left1'] == 0 == p['leftN'] for p in ps)
    for (name, takes) in (('B8-default-at', True), ('B8-default-above', False)):
        (seg, bands, nulls, S) = CASE[name].data()
        assert sc.default_takes_patches(seg.size, S) == takes
        assert seg.size == sc.MAXRUN * (S + 1) + (0 if takes else 1)


def test_every_part_of_the_issue_has_a_case():
    names = [c.name for c in sc.CASES]
    for part in ['A%d' % k for k in range(1, 10)] + ['B%d' % k for k in range(1, 9)]:
        assert any(n.startswith(part + '-') for n in names), part
    assert all(('flat' in c.entries) for c in sc.CASES)
    assert [c.name for c in sc.CASES if 'patch' not in c.entries] == ['A7-second-trip']
    assert sum(c.bands_extra for c in sc.CASES) == 1


@pytest.mark.parametrize('case', sc.CASES, ids=lambda c: c.name)
def test_model_and_bound_against_the_oracle(case, oracle):
    """the numpy model's integer columns are the oracle's, and the oracle's float columns stay within the bound"""
    (seg, bands, nulls, S) = case.data()
    want = sc.expected(case, oracle)
    names = sc.int_names(case.pcs)
    for (b, null) in enumerate(nulls):
        (ic, fc) = want[b]
        assert ic.dtype == np.int64 and fc.dtype == np.float32 and ic.shape == (len(names), S + 1)
        model = sc.int_model(seg, bands[b], null, S, case.missing, case.pcs)
        for (k, name) in enumerate(names):
            assert np.array_equal(model[name], ic[k]), (b, name)
        assert (ic[:, 0] == 0).all() and (fc[:, 0] == 0).all()
        assert sc.float_violations(seg, bands[b], null, S, case.missing, fc[0], fc[1]) == '', b
