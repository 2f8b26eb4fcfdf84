"""CPU: the cases and the model of tests/subset_cases.py.  visit_keys numbers every pixel once, the dict-loop model
equals the C oracle (the reference's visiting loop) on every case and the unmodified reference on its four goldens,
and the per-shard firsts merge to the model's numbering however the rows are split -- so what the kernels of
csrc/subset.h are compared with (tests/test_gpu_subset_edges.py) does not rest on one implementation."""
import numpy as np
import pytest

import subset_cases as sc


@pytest.mark.parametrize('ys,xs,T', sc.GEOMETRIES)
def test_visit_keys_is_a_permutation(ys, xs, T):
    keys = sc.visit_keys(ys, xs, T)
    assert keys.shape == (ys, xs)
    assert np.array_equal(np.sort(keys, axis=None), np.arange(ys * xs))
    # raster order inside a tile, tiles in raster order: a pixel comes after its left and upper neighbours in the
    # same tile, and after every pixel of the tile to the left and the tile row above
    for y in range(ys):
        for x in range(xs):
            if x % T:
                assert keys[y, x] == keys[y, x - 1] + 1
            elif x:
                assert keys[y, x] > keys[min(ys - 1, y // T * T + T - 1), x - 1]
            if y % T:
                assert keys[y, x] > keys[y - 1, x]
            elif y:
                assert keys[y, x] > keys[y - 1].max()


def test_cases_are_what_they_say():
    for c in sc.PERM_CASES:
        w = c.seg[c.tly:c.tly + c.ys, c.tlx:c.tlx + c.xs]
        assert np.array_equal(np.sort(w, axis=None), np.arange(1, c.xs * c.ys + 1))
        assert c.seg.shape == (c.tly + c.ys, c.tlx + c.xs)
    sizes = sorted({c.xs * c.ys for c in sc.WIDTH_CASES})
    assert sizes == [255, 256, 257, 65535, 65536, 65537]
    for c in sc.WIDTH_CASES:
        (out, orig, hist) = c.want()
        n = c.xs * c.ys
        if c.name.endswith('distinct'):
            assert len(orig) == n + 1 and (n < 65535 or n > max(sc.SORT_TILE, sc.SCAN_ITEMS))
        else:
            # id 1 only on the last pixel visited, and it is the last new id
            assert orig.tolist() == [0, 900, 500, 40, 1] and hist[4] == 1
            assert sc.visit_keys(c.ys, c.xs, c.T)[out == 4] == n - 1
    for c in sc.RANGE_CASES:
        present = np.unique(c.seg[c.tly:c.tly + c.ys, c.tlx:c.tlx + c.xs])
        assert set(sc.RANGE_IDS) <= set(present.tolist()) and present.max() <= c.max_seg_id
        assert c.seg.shape[1] > c.xs and c.tlx > 0 and c.tly > 0
    assert sorted({c.max_seg_id for c in sc.RANGE_CASES}) == [
        sc.SCAN_ITEMS + 1, sc.SCAN_ITEMS + 255, sc.SCAN_ITEMS + 256, sc.SCAN_ITEMS + 257, 1 << 20]
    for c in sc.SINGLE_ID_CASES:
        assert len(c.want()[1]) == 2 and c.want()[1][1] in (1, c.max_seg_id)
    for c in sc.BLOCKY_CASES:
        (out, orig, hist) = c.want()
        (_o, orig0, hist0) = sc.blocky_case(c.T, 'nomask').want()
        if 'hide-first' in c.name:
            # every id is still there with one pixel fewer, and none is first seen where it was
            assert sorted(orig.tolist()) == sorted(orig0.tolist())
            assert np.array_equal(np.sort(hist[1:]), np.sort(hist0[1:] - 1))
            firsts = sc.first_pixels(c.seg, *c.args)
            assert all(c.mask[p] == 1 for p in firsts.values())
            assert not set(firsts.values()) & set(sc.first_pixels(c.seg, *c.win, None, c.T).values())
        elif 'hide-ids' in c.name:
            assert len(orig) < len(orig0) and (orig[1:] % 3 != 0).all()
            assert np.array_equal(np.unique(out), np.arange(len(orig)))


@pytest.mark.parametrize('case', sc.ALL_CASES, ids=lambda c: c.name)
def test_model_equals_oracle(case, oracle):
    (out, orig, hist) = case.want()
    (want, worig, whist) = oracle.subset_recode(case.seg, case.tlx, case.tly, case.xs, case.ys, case.mask, case.T)
    assert np.array_equal(out, want)
    assert np.array_equal(orig, worig)
    assert np.array_equal(hist, whist)
    if case in sc.PERM_CASES:
        assert np.array_equal(out, sc.visit_keys(case.ys, case.xs, case.T) + 1) and (hist[1:] == 1).all()


@pytest.mark.parametrize('name,masked', [('a', False), ('b', True), ('c', False), ('d', True)])
def test_model_equals_reference_goldens(name, masked, golden):
    g = golden('subset_recode')
    (tlx, tly, xs, ys, tile) = [int(v) for v in g[name + '_win']]
    mask = (g['mask'] != 0).astype(np.uint8) if masked else None
    (out, orig, hist) = sc.model(g['seg'], tlx, tly, xs, ys, mask, tile)
    assert np.array_equal(out, g[name + '_out'])
    assert np.array_equal(orig, g[name + '_orig'])
    assert np.array_equal(hist, g[name + '_hist'])


def _splits(ys):
    rng = np.random.RandomState(sc._seed('splits'))
    yield [0, ys]
    yield list(range(ys + 1))
    for _ in range(6):
        cuts = np.sort(rng.randint(0, ys + 1, size=rng.randint(1, 6))).tolist()
        yield [0] + cuts + [ys]                 # empty shards included


@pytest.mark.parametrize('case', list(sc.SHARD_CASES.values()) + sc.BLOCKY_CASES + sc.RANGE_CASES[:1],
                         ids=lambda c: c.name)
def test_shard_firsts_merge_to_the_model(case):
    (_out, orig, _hist) = case.want()
    for cuts in _splits(case.ys):
        parts = [sc.shard_first(case.seg, *case.args, rows=(a, b)) for (a, b) in zip(cuts, cuts[1:])]
        for (keys, ids) in parts:
            assert (np.diff(ids.astype(np.int64)) > 0).all() and len(keys) == len(ids)
        assert np.array_equal(sc.merge_first(parts), orig), cuts
    # in reverse, and with a shard given twice: a minimum does not care
    assert np.array_equal(sc.merge_first(parts[::-1] + parts[:1]), orig)


@pytest.mark.parametrize('T', sc.SHARD_TILES)
def test_shard_layouts(T):
    (tlx, tly, xs, ys) = sc.SHARD_WIN
    for layout in sc.SHARD_LAYOUTS:
        cuts = sc.shard_cuts(layout, T)
        assert cuts[0] == 0 and cuts[-1] == sc.SHARD_ROWS and cuts == sorted(cuts)
        held = [sc.held_rows(lo, hi, tly, ys) for (lo, hi) in zip(cuts, cuts[1:])]
        cover = np.zeros(ys, dtype=int)
        for (a, b) in held:
            cover[a:b] += 1
        assert (cover == 1).all()
        starts = {a for (a, b) in held if b > a}
        if layout in ('on-tile-row', 'row-above', 'row-below'):
            d = {'on-tile-row': 0, 'row-above': -1, 'row-below': 1}[layout]
            assert 2 * T + d in starts and (2 * T + d) % T == d % T
        elif layout == 'single-rows':
            assert all(b - a <= 1 for (a, b) in held) and len(starts) == ys
        elif layout == 'above-and-below':
            assert held[0] == (0, 0) and held[-1] == (ys, ys) and cuts[1] > 0 and cuts[-2] < sc.SHARD_ROWS
        else:
            assert held == [(0, ys)]


def test_hand_built_pairs():
    (words, counts) = sc.gathered_pairs()
    parts = []
    for r, n in enumerate(counts.tolist()):
        slot = words[r * 2 * sc.PAIRS_SLOT:(r + 1) * 2 * sc.PAIRS_SLOT]
        parts.append((slot[:n], slot[n:2 * n]))
        assert (slot[2 * n:] == sc.PAIRS_PAD).all() and n < sc.PAIRS_SLOT
    assert 0 in counts and max(k for (keys, _i) in sc.PAIRS_RANKS for k in keys) < sc.PAIRS_WIN[0] * sc.PAIRS_WIN[1]
    assert sc.merge_first(parts, sc.PAIRS_MAX_ID).tolist() == list(sc.PAIRS_ORIG)
    # the padding read as pairs would move id PAIRS_PAD to the front
    pad = (np.array([sc.PAIRS_PAD], np.uint32), np.array([sc.PAIRS_PAD], np.uint32))
    assert sc.merge_first(parts + [pad], sc.PAIRS_MAX_ID).tolist() != list(sc.PAIRS_ORIG)
    # id 7's minimum is on the last rank, and some rank's keys are not sorted
    mins = [min([k for (k, s) in zip(*p) if s == 7] or [1 << 40]) for p in sc.PAIRS_RANKS]
    assert mins.index(min(mins)) == len(sc.PAIRS_RANKS) - 1 and sum(m < (1 << 40) for m in mins) == 3
    assert any(list(keys) != sorted(keys) for (keys, _i) in sc.PAIRS_RANKS)
