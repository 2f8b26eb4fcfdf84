"""CPU: the oracle's per-segment tables against independent numpy restatements, on every generator of
tests/segtable_cases.py, before the GPU tests of those tables (tests/test_gpu_segment_tables.py) rely on
the oracle.

  spectra    np.add.at(acc_f32, seg, band.astype(float64)): unbuffered, raster order, each add the
             float32 rounding of float32 + float64 -- the reference's `float32 + pixel`
  locations  np.argsort(seg, kind='stable'): pixels grouped by id, raster order inside a segment
"""
import numpy as np
import pytest

import segtable_cases as sc


def _nb(case):
    return 2 if 2 in case.nbs else case.nbs[0]


@pytest.mark.parametrize('case', sc.CASES, ids=[c.name for c in sc.CASES])
def test_oracle_spectra_equal_numpy_restatement(case, oracle):
    for dtype in case.dtypes:
        seg, img, S = sc.make(case, dtype, _nb(case))
        want = sc.restated_spectra(seg, img, S)
        got = oracle.build_segment_spectra(seg, img, S)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (case.name, dtype)
        # below the bound the float32 sum is the exact integer sum
        tot, absum = sc.int_sums(seg, img, S)
        small = absum < sc.LIM
        assert np.array_equal(got[small].astype(np.int64), tot[small]), (case.name, dtype)


@pytest.mark.parametrize('case', sc.CASES, ids=[c.name for c in sc.CASES])
def test_oracle_locations_equal_stable_argsort(case, oracle):
    seg, S = case.seg()
    off, rc = oracle.segment_locations(seg, S)
    order = np.argsort(seg.ravel(), kind='stable').astype(np.int64)
    nnull = int((seg == 0).sum())
    want = order[nnull:]                                   # the oracle omits the null segment
    assert np.array_equal(rc[:, 0].astype(np.int64) * seg.shape[1] + rc[:, 1], want), case.name
    cnt = np.bincount(seg.ravel(), minlength=S + 1)
    cnt[0] = 0
    assert np.array_equal(off.astype(np.int64), np.r_[0, np.cumsum(cnt)]), case.name


def test_generators_cover_the_issue_list():
    """the generators reach what the GPU tests need: every size, the radix sort with 1, 2, 3 and 4 passes
    (the pass count decides which ping-pong buffer the pixel list ends in), > 16 384 big segments, a large
    null segment, ids without pixels and max_seg_id above the largest id"""
    sizes, passes = set(), set()
    for c in sc.CASES:
        seg, S = c.seg()
        cnt = np.bincount(seg.ravel(), minlength=S + 1)
        sizes |= set(cnt[1:].tolist())
        passes.add(sc.radix_passes(S))
    assert set(sc.SIZES) <= sizes
    assert any(s >= 10 ** 6 for s in sizes)
    assert passes == {1, 2, 3, 4}
    seg, S = sc.BY_NAME['many_big'].seg()
    assert (np.bincount(seg.ravel())[1:] > 64).sum() > sc.SPECTRA_GRID_SLOTS
    seg, S = sc.BY_NAME['null_big'].seg()
    assert (seg == 0).sum() > 10 ** 5
    seg, S = sc.BY_NAME['ids_257'].seg()
    assert S > int(seg.max()) and (np.bincount(seg.ravel(), minlength=S + 1)[1:] == 0).any()
    seg, S = sc.BY_NAME['odd_shape'].seg()
    assert seg.size % 4 and seg.size % 64 and seg.size % 4096


def test_spectra_regimes_reach_both_phases():
    """for every pixel type some segments above 64 pixels stay below the 2^24 bound and some cross it, so
    both the exact and the ordered phase of k_spectra_big run; the crossing cases cross where they say"""
    for dtype in sc.DTYPES:
        below = above = False
        for case in sc.CASES:
            if dtype not in case.dtypes:
                continue
            seg, img, S = sc.make(case, dtype, 1)
            cnt = np.bincount(seg.ravel(), minlength=S + 1)
            _tot, absum = sc.int_sums(seg, img, S)
            big = cnt > 64
            below |= bool((big & (absum[:, 0] < sc.LIM)).any())
            above |= bool((big & (absum[:, 0] >= sc.LIM)).any())
        assert below and above, dtype
    # 16384 per pixel: sum(|v|) = 2^24 exactly after 1024 pixels (the end of the second 512-pixel chunk)
    assert 16384 * 1024 == sc.LIM and 65535 * 256 < sc.LIM < 65535 * 257 and 255 * 65793 < sc.LIM <= 255 * 65794
