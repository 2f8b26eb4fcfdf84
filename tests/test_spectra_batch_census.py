"""What tests/spectra_batch_cases.py claims about its raster, asserted on the CPU from the oracle's cluster codes and
clumps: every tile window holds segments above 64 pixels of each kind the spectra kernel for them
(csrc/elim_small.h k_spectra_big) treats differently, on both sides of the 2^24 bound of its exact phase."""
import numpy as np
import pytest

import spectra_batch_cases as sbc

_census = {}


def census(oracle, dtype, nb, four):
    """per tile window in sorted tile-key order: (sizes, bound sums) of its clumps, where a clump's bound sum is the
    sum over its pixels of the largest band value: what the kernel's exact phase keeps below 2^24"""
    key = (dtype, nb, bool(four))
    if key not in _census:
        img, cen = sbc.image(dtype, nb)
        tiles, _ntc, _ntr = oracle.get_tiles(sbc.NR, sbc.NC, sbc.TILE, sbc.OVERLAP)
        out = []
        for k in sorted(tiles):
            (x, y, xs, ys) = tiles[k]
            sub = np.ascontiguousarray(img[:, y:y + ys, x:x + xs])
            cl = oracle.kmeans_assign(sub, cen).astype(np.int32)
            assert np.array_equal(cl, sbc.codes()[y:y + ys, x:x + xs])
            seg, nxt = oracle.clump(cl, 0, four, 1)
            sizes = np.bincount(seg.ravel(), minlength=nxt)[1:]
            bound = np.bincount(seg.ravel(), weights=sub.max(axis=0).ravel().astype(np.float64), minlength=nxt)[1:]
            out.append((sizes, bound))
        _census[key] = out
    return _census[key]


def test_four_tile_windows(oracle):
    tiles, ntc, ntr = oracle.get_tiles(sbc.NR, sbc.NC, sbc.TILE, sbc.OVERLAP)
    assert (ntc, ntr, len(tiles)) == (4, 1, 4)


@pytest.mark.parametrize('dtype,nb,four', [('uint16', 6, True), ('uint16', 6, False), ('uint16', 10, True)])
def test_every_tile_holds_every_kind(oracle, dtype, nb, four):
    for (sizes, bound) in census(oracle, dtype, nb, four):
        # no single pixels: the single-pixel stage leaves the clumps as drawn; some below minSegmentSize: a pass loop
        assert sizes.min() > 1 and (sizes < sbc.MINSEG).any()
        hi = bound >= sbc.BOUND
        # 65 pixels never reach 2^24 at 16 bits; 512 and 513 do with values near 65535 (their first group already:
        # all of their sum is ordered) and do not with values below 1500
        assert ((sizes == sbc.BIG + 1) & ~hi).sum() >= 2
        for want in (sbc.EXACT_GROUP, sbc.EXACT_GROUP + 1):
            assert ((sizes == want) & ~hi).sum() >= 1 and ((sizes == want) & hi).sum() >= 1, want
        stripes = (sizes > 9000) & (sizes < 11000)
        top = stripes & (bound / sizes > 60000)
        assert top.sum() >= 3 and (stripes & ~hi).sum() >= 3
        # values near 65535 pass the bound after ~260 pixels: the ordered phase does most of those pieces' work
        assert hi[top].all() and (bound[top] / sizes[top]).min() * 270 > sbc.BOUND
        # and the values of the low ones are below 1500
        assert (bound[stripes & ~hi] / sizes[stripes & ~hi]).max() < 1500


def test_uint8_twin_has_the_same_segments(oracle):
    a = census(oracle, 'uint8', 6, True)
    b = census(oracle, 'uint16', 6, True)
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(a, b))
