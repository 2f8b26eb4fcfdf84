"""The spatial-statistics cases of spatial_cases.py on the CPU: the oracle against the unmodified reference on
wide 32-bit imagery (tests/golden/spatial_wide.npz), and the integer formula the device adds squares with
against the oracle -- it must fail on every wide case, or the cases stopped testing the recompute."""
import zlib

import numpy as np
import pytest

import spatial_cases as sc

MISSING = -9999


def _same(got, want):
    """bit for bit, NaN included"""
    return np.array_equal(np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32))


def test_cases_are_deterministic_and_cover_the_regimes():
    for name in sc.CASES:
        (seg, band, null, S) = sc.CASES[name].make()
        assert seg.dtype == np.uint32 and band.dtype == sc.CASES[name].dtype and seg.shape == band.shape
        assert int(seg.max()) <= S
        for again in (sc._make.__wrapped__(name), sc._make.__wrapped__(name)):     # uncached: built afresh
            assert np.array_equal(again[0], seg) and np.array_equal(again[1], band), name
            assert again[2:] == (null, S), name
    (seg, band, null, S) = sc.CASES['u16_big'].make()
    assert int((seg == 1).sum()) >= 10 ** 6
    for name in sc.WIDE:
        (seg, band, null, S) = sc.CASES[name].make()
        v = band.astype(np.int64)[band != null]
        assert int(v.max()) - int(v.min()) > 94906265           # some square of a difference reaches 2^53
    for name in ('i32_full', 'u32_full', 'i32_extreme_nullmin', 'u32_extreme_nullmax'):
        (seg, band, null, S) = sc.CASES[name].make()
        v = band.astype(np.int64)[band != null]
        assert int(v.max()) - int(v.min()) > 3037000499         # the reference's int64 square wraps


def test_wrapped_sums_give_nan(oracle):
    """limits only: every square of a non-zero difference wraps negative, so bin sums do too -> NaN"""
    for name in ('i32_extreme_nullmin', 'u32_extreme_nullmax'):
        (seg, band, null, S) = sc.CASES[name].make()
        _i, fc = oracle.spatialstats(seg, band, 'variogram', 5, null, 0, 5, max_seg_id=S)
        assert np.isnan(fc).any()


def test_oracle_matches_reference_wide_golden(golden, oracle):
    g = golden('spatial_wide')
    maxd, tile, tr = int(g['maxd']), int(g['tile']), g['transform']
    for name in [str(x) for x in g['cases']]:
        (seg, band, null, S) = sc.CASES[name].make()
        assert int(g[name + '_crc']) == zlib.crc32(seg.tobytes()) ^ zlib.crc32(band.tobytes()), name
        n = g[name + '_vario_fc'].shape[1]          # the reference's columns end at the largest id present
        _i, fc = oracle.spatialstats(seg, band, 'meancoord', tr, null, 0, 2, tile_size=tile, max_seg_id=S)
        assert _same(fc[:, :n], g[name + '_mean_fc']), name
        assert (fc[:, n:] == MISSING).all()
        for (four, key) in ((1, 'edge4_ic'), (0, 'edge8_ic')):
            ic, _f = oracle.spatialstats(seg, band, 'numedge', four, null, 1, 0, tile_size=tile, max_seg_id=S)
            assert np.array_equal(ic[:, :n], g['%s_%s' % (name, key)]), (name, key)
        _i, fc = oracle.spatialstats(seg, band, 'variogram', maxd, null, 0, maxd, tile_size=tile, max_seg_id=S)
        assert _same(fc[:, :n], g[name + '_vario_fc']), name


def _model_vs_oracle(oracle, name, maxd):
    (seg, band, null, S) = sc.CASES[name].make()
    model, sums, cnts = sc.int_model_variogram(seg, band, null, maxd, S)
    _i, fc = oracle.spatialstats(seg, band, 'variogram', maxd, null, 0, maxd, max_seg_id=S)
    held = cnts > 0
    assert (fc[:, 0] == 0).all() and (fc[:, 1:][~held[:, 1:]] == MISSING).all()
    return model[held].view(np.uint32) != fc[held].view(np.uint32), sums[held]


def test_chain_tells_the_reference_order_from_any_other(oracle):
    """On the chain only the reference's sequential float64 sum gives the oracle's value: the exact sum, the
    reversed order and numpy's pairwise sum all give other float32 bits, so a recompute in any of those orders
    (or of the ranks' parts in the wrong order) fails the GPU tests."""
    (seg, band, null, S) = sc.CASES['u32_chain'].make()
    _i, fc = oracle.spatialstats(seg, band, 'variogram', 1, null, 0, 1, max_seg_id=S)
    iterms = sc.reference_terms(seg, band, null, 1, 2, 1)
    assert len(iterms) == len(sc.CHAIN) - 1
    terms = iterms.astype(np.float64)

    def value(total):
        return np.float32(np.sqrt(total / len(terms)))
    exact = float(sum(int(t) for t in iterms))         # the int64 terms added exactly, rounded once
    assert value(np.cumsum(terms)[-1]).view(np.uint32) == fc[0, 2].view(np.uint32)
    others = {'exact': value(exact), 'reversed': value(np.cumsum(terms[::-1])[-1]), 'pairwise': value(np.sum(terms))}
    for (how, v) in others.items():
        assert v.view(np.uint32) != fc[0, 2].view(np.uint32), how
    assert len({v.view(np.uint32) for v in others.values()} | {fc[0, 2].view(np.uint32)}) == 4


@pytest.mark.parametrize('name', sc.WIDE)
def test_integer_formula_fails_every_wide_case(oracle, name):
    maxd = min(sc.CASES[name].maxds)
    diff, sums = _model_vs_oracle(oracle, name, maxd)
    assert diff.any(), "the integer variogram matches the reference on %s: the case no longer tests the recompute" % name


@pytest.mark.parametrize('name', sc.NARROW)
def test_integer_formula_is_exact_on_narrow_cases(oracle, name):
    maxd = min(sc.CASES[name].maxds)
    diff, sums = _model_vs_oracle(oracle, name, maxd)
    assert (sums < sc.EXACT).all() and not diff.any()


def test_big_segment_passes_2_53_with_exact_squares():
    (seg, band, null, S) = sc.CASES['u16_big'].make()
    model, sums, cnts = sc.int_model_variogram(seg, band, null, 5, S)
    assert (sums[:, 1] >= sc.EXACT).any() and (sums[:, 1] < (1 << 63)).all()
