"""CPU: the generated stitch cases (tests/stitch_cases.py).  The numpy model of the stitch equals the C
oracle on every case and the unmodified reference on its five golden tilings, and every case reaches
what it was built to reach (the census conditions)."""
import numpy as np
import pytest

import stitch_cases as sc

NAMES = [c.name for c in sc.all_cases()]
GOLDEN_STITCH = ['stitch_2x2', 'stitch_3x3_null', 'stitch_3x4_8conn', 'stitch_quirk_empties', 'stitch_quirk_zeros']


def _vs_oracle(case, oracle, simple):
    m = sc.model_stitch(case, simple=simple)
    (out, mx, hist) = oracle.stitch_tiles(case.tiles, case.geom, case.ntc, case.ntr, case.nr, case.nc,
                                          case.overlap, simple=simple)
    assert mx == m.maxSegId
    assert np.array_equal(out, m.mosaic)
    assert np.array_equal(hist, m.hist)
    return m


@pytest.mark.parametrize('name', NAMES)
def test_model_equals_oracle(name, oracle):
    case = sc.case(name)
    for (col, row) in case.tiles:
        t = case.tiles[(col, row)]
        assert np.array_equal(np.unique(t[t != 0]), np.arange(1, int(t.max()) + 1)), 'ids with gaps'
        assert max(t.shape) <= 240
    m = _vs_oracle(case, oracle, False)
    for (col, row) in case.order():
        res = m.tiles[(col, row)]
        (top, bottom, left, right, _x, _y) = case.window(col, row)
        got = oracle.recode_tile(case.tiles[(col, row)], case.overlap,
                                 m.tiles[(col, row - 1)].bottom if row > 0 else None,
                                 m.tiles[(col - 1, row)].right if col > 0 else None, res.base, top, bottom, left, right)
        assert np.array_equal(got, res.recoded), (col, row)


@pytest.mark.parametrize('name', ['ties/3x3', 'random/05'])
def test_model_equals_oracle_simple(name, oracle):
    _vs_oracle(sc.case(name), oracle, True)


@pytest.mark.parametrize('name', GOLDEN_STITCH)
def test_model_equals_reference_goldens(name, golden, oracle):
    """the model on oracle-segmented tiles against the mosaics the reference itself stitched"""
    g = golden(name)
    (nr, nc) = g['mosaic'].shape
    (tile, ov) = (int(g['tile_size']), int(g['overlap']))
    (tiles, _c, _r) = oracle.get_tiles(nr, nc, tile, ov)
    null = int(g['null_val']) if int(g['has_null']) else None
    local = {}
    for ((c, r), (x, y, xs, ys)) in tiles.items():
        sub = np.ascontiguousarray(g['img'][:, y:y + ys, x:x + xs])
        local[(c, r)] = oracle.segment_tile(sub, g['centres'], int(g['min_seg']), float(g['msd']), null,
                                            bool(g['four']))['segimg']
    case = sc.Case('golden', name, nr, nc, tile, ov, local, seed=0, four=bool(g['four']))
    m = sc.model_stitch(case)
    assert m.maxSegId == int(g['max_seg_id'])
    assert np.array_equal(m.mosaic, g['mosaic'])
    assert np.array_equal(m.hist, g['hist'])


def test_mode_equals_scipy():
    """the model's mode (numpy.unique, the smallest of the most frequent) is scipy.stats.mode, as the
    reference calls it (tiling.py:1194-1200), on every crossing segment of the `ties` tilings"""
    stats = pytest.importorskip('scipy.stats')
    n = 0
    for case in sc.group('ties'):
        m = sc.model_stitch(case)
        o = case.overlap
        for (col, row) in case.order():
            (tile, res) = (case.tiles[(col, row)], m.tiles[(col, row)])
            for (modes, A, B) in ((res.modes_top, tile[:o, :], m.tiles[(col, row - 1)].bottom if row > 0 else None),
                                  (res.modes_left, tile[:, :o], m.tiles[(col - 1, row)].right if col > 0 else None)):
                for (s, want) in modes.items():
                    got = stats.mode(B[A == s])
                    got = got.mode if np.isscalar(got.mode) else got.mode[0]
                    assert int(got) == want
                    n += 1
    assert n >= 100


# ---- the census conditions: what every group must reach ----------------------------------------
def test_census_ties():
    assert [(c.ntc, c.ntr, c.overlap) for c in sc.group('ties')] == [(2, 2, 16), (3, 3, 16)]
    t = sc.group_census('ties')
    assert t['ties'] >= 20 and t['ties_zero'] >= 5 and t['ties3'] >= 1
    assert t['tie_win_hi_slot'] >= 1 and t['tie_win_lo_slot'] >= 1


def test_census_midline():
    cases = sc.group('midline')
    assert [c.overlap for c in cases] == [2, 3, 7, 16, 17, 1]
    for c in cases:
        cen = sc.model_stitch(c).census
        assert (c.ntc, c.ntr) == (2, 2)
        for s in ('top', 'left'):
            if c.overlap == 1:                          # mid = 0: nothing can lie before it
                assert cen[s + '_crossing'] == 0 and cen[s + '_starts_at'] >= 1
            else:
                assert cen[s + '_ends_before'] >= 1 and cen[s + '_starts_at'] >= 1, (c.name, s)
                assert cen[s + '_spans'] >= 1 and cen[s + '_crossing'] > cen[s + '_spans'] // 2, (c.name, s)


def test_census_both_strips():
    t = sc.group_census('both_strips')
    assert t['overrides'] >= 5 and t['cross_both'] > t['overrides'] // 2
    assert t['cross_top_only'] >= 1 and t['cross_left_only'] >= 1


def test_census_shapes():
    """every shape crosses the top strip's midline somewhere, the left strip's somewhere, and somewhere has
    pixels on both sides of an edge of the trimmed window"""
    (case,) = sc.group('shapes')
    m = sc.model_stitch(case)
    seen = {}
    for ((col, row), stamps) in case.stamped.items():
        (tile, res) = (case.tiles[(col, row)], m.tiles[(col, row)])
        (top, bottom, left, right, _x, _y) = case.window(col, row)
        for (kind, r0, c0, mask) in stamps:
            (rr, cc) = np.nonzero(mask)
            s = int(tile[r0 + rr[0], c0 + cc[0]])
            assert np.array_equal(tile == s, _placed(tile.shape, r0, c0, mask)), 'a shape was cut'
            inside = (rr + r0 >= top) & (rr + r0 < bottom) & (cc + c0 >= left) & (cc + c0 < right)
            k = seen.setdefault(kind, set())
            if res.cross_top[s]:
                k.add('top')
            if res.cross_left[s]:
                k.add('left')
            if inside.any() and not inside.all():
                k.add('window')
    assert sorted(seen) == ['U', 'comb', 'diag', 'pieces', 'ring', 'stair8']
    for (kind, k) in seen.items():
        assert k == {'top', 'left', 'window'}, (kind, k)


def _placed(shape, r0, c0, mask):
    a = np.zeros(shape, dtype=bool)
    a[r0:r0 + mask.shape[0], c0:c0 + mask.shape[1]] = mask
    return a


def _extents(A):
    """per id of a strip: first / last row and first / last column"""
    (rr, cc) = np.nonzero(A)
    lab = A[rr, cc]
    n = int(A.max()) + 1
    out = []
    for (v, f) in ((rr, np.minimum), (rr, np.maximum), (cc, np.minimum), (cc, np.maximum)):
        e = np.full(n, sc.BIG if f is np.minimum else -1, dtype=np.int64)
        f.at(e, lab, v)
        out.append(set(e[np.unique(lab)].tolist()))
    return out


def test_census_lane_edges():
    cases = sc.group('lane_edges')
    assert sorted(c.overlap for c in cases) == [16, 24]
    widths = set()
    top = [set(), set(), set(), set()]                  # over every top strip: first / last rows, first / last columns
    left = [set(), set(), set(), set()]
    for c in cases:
        m = sc.model_stitch(c)
        o = c.overlap
        for ((col, row), tile) in c.tiles.items():
            widths.add(tile.shape[1])
            if row > 0:
                top = [a | b for (a, b) in zip(top, _extents(tile[:o, :]))]
                assert m.tiles[(col, row)].cross_top.sum() >= 1
            if col > 0:
                left = [a | b for (a, b) in zip(left, _extents(tile[:, :o]))]
                assert m.tiles[(col, row)].cross_left.sum() >= 1
    assert {70, 130} <= widths
    assert {7, 8} <= top[0] and {7, 8} <= top[1]
    assert {63, 64, 127, 128} <= top[2] and {63, 64, 127, 128} <= top[3]
    assert {7, 8, 31, 32} <= left[0] and {7, 8, 31, 32} <= left[1]
    t = sc.group_census('lane_edges')
    assert t['row_continuations'] >= 8 and t['top_crossing'] >= 20 and t['left_crossing'] >= 20


def test_census_outside_owner():
    (case,) = sc.group('outside_owner')
    cen = sc.model_stitch(case).census
    assert cen['outside_new'] >= 3
    assert cen['k_ne_r_tiles'] == [(0, 0)]
    res = sc.model_stitch(case).tiles[(0, 0)]
    assert res.K - res.R >= 3


def test_census_dense_pairs():
    (case,) = sc.group('dense_pairs')
    m = sc.model_stitch(case)
    res = m.tiles[(1, 1)]
    (ys, xs) = case.tiles[(1, 1)].shape
    o = case.overlap
    assert res.cross_px == [(xs - o) * o, (ys - o) * o]     # every strip pixel outside the corner crosses ..
    assert m.census['dense_strips'] == 2                    # .. and each has a (segment, neighbour id) pair of its own
    assert sc.table_size(case, ys, xs, True, True, res.cross_px) == 2048       # 992 pairs: the table's highest load


def test_census_many_segments():
    (case,) = sc.group('many_segments')
    m = sc.model_stitch(case)
    assert case.tiles[(1, 1)].shape == (192, 192) and (case.ntc, case.ntr) == (2, 2)
    res = m.tiles[(1, 1)]
    assert len(res.lut) - 1 > 8192 and res.own[8192:].sum() > 100 and res.own[:8192].sum() > 100
    assert (res.cross_top[8192:].any() or res.cross_left[8192:].any())
    assert m.census['max_ids_per_patch'] > 128


def test_census_grids_and_random():
    g = {c.name: c for c in sc.group('grids')}
    assert g['grids/1xN'].ntr == 1 and g['grids/1xN'].ntc >= 3
    assert g['grids/Nx1'].ntc == 1 and g['grids/Nx1'].ntr >= 3
    c = g['grids/grown']
    (_x, _y, xs, ys) = c.geom[(c.ntc - 1, c.ntr - 1)]
    assert xs > c.tile and ys > c.tile and c.ntc >= 3 and c.ntr >= 3
    r = sc.group('random')
    assert len(r) == 20
    assert {c.tile for c in r} <= {32, 40, 48} and {c.overlap for c in r} <= {3, 4, 7, 8, 16}
    assert all(60 <= c.nr <= 140 and 60 <= c.nc <= 140 for c in r)
    nulls = np.mean([np.mean(t == 0) for c in r for t in c.tiles.values()])
    assert 0.02 < nulls < 0.04
    t = sc.group_census('random')
    assert t['ties'] >= 20 and t['overrides'] >= 5


def test_docstring_holds_the_census():
    assert sc.census_table() in sc.__doc__
