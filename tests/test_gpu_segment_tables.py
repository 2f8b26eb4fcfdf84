"""GPU: the per-segment tables of the elimination stage, compared directly on every generator of
tests/segtable_cases.py -- not only through the labels they lead to.

  spectra    buildSegmentSpectra (k_spectra_small / k_spectra_small_grp, k_big_seg_list, k_spectra_big)
             bit for bit against the oracle at five pixel types x nb 1..8, 9, 12, 16, 17 (band groups of
             BG = 1..8, and the multi-pass forms for nb > 8); against the numpy restatement of
             tests/test_oracle_spectra_restatement.py where it runs quickly; and equal to the exact integer
             sum wherever sum(|v|) of a segment's band stays below 2^24
  locations  shp_segment_locations (csr.h: runs of <= 64 pixels through the radix sort, 1..4 passes)
             against the oracle and a stable argsort, the null segment's entries included
  sizes      makeSegSize against np.bincount
  2^26       the runs path at n = 2^26 and the pixel-sort fallback just above it
"""
import numpy as np
import pytest

import knob_cases
import segtable_cases as sc

pytestmark = pytest.mark.gpu

RESTATE_MAX = 2_000_000          # band-pixels up to which the numpy restatement runs too


@pytest.fixture(scope='module')
def shepseg():
    from pyshepseg_amd import shepseg as m
    from pyshepseg_amd import _lib
    assert _lib.lib().shp_device_count() > 0, 'no GPU: the HIP path cannot run'
    return m


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('case', sc.CASES, ids=[c.name for c in sc.CASES])
def test_spectra_every_dtype_and_band_count(case, shepseg, oracle):
    nbmax = max(case.nbs)
    for dtype in case.dtypes:
        seg, img, S = sc.make(case, dtype, nbmax)          # band b's values do not depend on nb
        tot, absum = sc.int_sums(seg, img, S)
        exact = absum < sc.LIM
        restated = sc.restated_spectra(seg, img, S) if seg.size * nbmax <= RESTATE_MAX else None
        for nb in case.nbs:
            sub = img[:nb]
            got = shepseg.buildSegmentSpectra(seg, sub, S)
            assert got.dtype == np.float32 and got.shape == (S + 1, nb)
            want = oracle.build_segment_spectra(seg, sub, S)
            bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
            assert bad.size == 0, '%s %s nb=%d: %d segments differ from the oracle, first %s: %r != %r' % (
                case.name, dtype, nb, bad.size, bad[:5], got[bad[0]], want[bad[0]])
            if restated is not None:
                assert np.array_equal(_bits(got), _bits(restated[:, :nb])), (case.name, dtype, nb)
            ex = exact[:, :nb]
            assert np.array_equal(got[ex].astype(np.int64), tot[:, :nb][ex]), (case.name, dtype, nb)


@pytest.mark.parametrize('case', sc.CASES, ids=[c.name for c in sc.CASES])
def test_locations_and_sizes(case, shepseg, oracle):
    seg, S = case.seg()
    got = knob_cases.device_tables(seg, None, S)
    want = knob_cases.expected_tables(seg, None, S, oracle)
    assert np.array_equal(got['off'], want['off']), case.name
    assert np.array_equal(got['pix'], want['pix']), case.name
    assert np.array_equal(got['size'], want['size']), case.name
    # the oracle's locations (null pixels omitted) and the null segment's entries
    woff, wrc = oracle.segment_locations(seg, S)
    nnull = int(got['off'][1])
    assert np.array_equal(got['off'][1:].astype(np.int64) - nnull, woff[1:].astype(np.int64)), case.name
    lin = wrc[:, 0].astype(np.int64) * seg.shape[1] + wrc[:, 1]
    assert np.array_equal(got['pix'][nnull:].astype(np.int64), lin), case.name
    assert np.array_equal(got['pix'][:nnull].astype(np.int64), np.flatnonzero(seg.ravel() == 0)), case.name


def _boundary_raster(nr, nc):
    """uint32 ids of 8 x 100 blocks (about 84 000 segments: 3 radix passes), a 100-row null band, and a
    one-band uint8 image whose null band sums far past 2^24"""
    r = np.arange(nr, dtype=np.uint32)
    c = np.arange(nc, dtype=np.uint32)
    seg = (r[:, None] // np.uint32(8)) * np.uint32(83) + (c[None, :] // np.uint32(100)) + np.uint32(1)
    seg[4000:4100] = 0
    img = ((r[:, None] * np.uint32(7) + c[None, :] * np.uint32(13)) % np.uint32(251)).astype(np.uint8)
    return seg, img[None]


@pytest.mark.parametrize('nr', [8192, 8193], ids=['runs_n_2p26', 'pixel_sort_above_2p26'])
def test_csr_boundary_2p26(nr, shepseg, oracle):
    """n = 2^26 pixels is the largest raster the runs path takes (a run's start is stored in 26 bits);
    n = 2^26 + 8192 falls back to the plain pixel sort.  Locations, sizes and one-band spectra against
    the oracle.  Needs about 2 GB of host memory (raster, pixel list, the oracle's row/col pairs)."""
    nc = 8192
    seg, img = _boundary_raster(nr, nc)
    assert (seg.size <= 1 << sc.RUN_POS_BITS) == (nr == 8192)
    S = int(seg.max())
    assert sc.radix_passes(S) == 3
    got = knob_cases.device_tables(seg, img, S)
    assert np.array_equal(_bits(got['spectra']), _bits(oracle.build_segment_spectra(seg, img, S)))
    cnt = np.bincount(seg.ravel(), minlength=S + 1)
    assert np.array_equal(got['size'], cnt.astype(np.uint32))
    assert np.array_equal(got['off'][1:].astype(np.int64), np.cumsum(cnt))
    nnull = int(cnt[0])
    assert np.array_equal(got['pix'][:nnull], np.flatnonzero(seg.ravel() == 0).astype(np.uint32))
    del cnt
    woff, wrc = oracle.segment_locations(seg, S)
    assert np.array_equal(got['off'][1:].astype(np.int64) - nnull, woff[1:].astype(np.int64))
    del woff
    lin = wrc[:, 0] * np.uint32(nc)
    lin += wrc[:, 1]
    del wrc
    assert np.array_equal(got['pix'][nnull:], lin)
