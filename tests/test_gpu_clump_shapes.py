"""GPU: the depth-first cut replay (pyshepseg_amd/csrc/clump.h) on the shapes of tests/clump_shape_cases.py,
whose walks reach every step of the walker (tests/test_clump_shapes_host.py asserts that they do), against the C
oracle: labels and next id, exactly.  Plain, and inside a null margin that takes every component off the raster
edges and its rows off word alignment.  Then the fused pipeline on three of them, so that the one-pixel pieces of
a cut component reach the single-pixel stage and the cut pieces the small-segment stage."""
import numpy as np
import pytest

import clump_shape_cases as cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def shepseg():
    from pyshepseg_amd import shepseg as m
    from pyshepseg_amd import _lib
    assert _lib.lib().shp_device_count() > 0, 'no GPU: the HIP path cannot run'
    return m


def _first_difference(seg, oseg):
    """where the labels first differ in raster order, and the oracle's piece there (its seed and size)"""
    d = np.flatnonzero(seg.ravel() != oseg.ravel())
    if d.size == 0:
        return 'labels equal'
    (r, c) = divmod(int(d[0]), seg.shape[1])
    piece = oseg == oseg[r, c]
    (sr, sc) = divmod(int(np.flatnonzero(piece.ravel())[0]), seg.shape[1])
    return '%d pixels differ, first at (%d, %d): got %d, want %d (piece seeded at (%d, %d), %d pixels)' % (
        d.size, r, c, seg[r, c], oseg[r, c], sr, sc, int(piece.sum()))


def _check(shepseg, oracle, cl, four):
    seg, nxt = shepseg.clump(cl, 0, fourConnected=four)
    oseg, onxt = oracle.clump(cl, 0, four, 1)
    assert seg.dtype == np.uint32 and seg.shape == oseg.shape
    assert np.array_equal(seg, oseg), _first_difference(seg, oseg)
    assert nxt == onxt


@pytest.mark.parametrize('pad', [False, True], ids=['plain', 'padded'])
@pytest.mark.parametrize('four', [True, False], ids=['4conn', '8conn'])
@pytest.mark.parametrize('name', cs.MODEL_SHAPES)
def test_clump_shape_matches_oracle(name, four, pad, shepseg, oracle):
    cl = cs.make(name)
    _check(shepseg, oracle, cs.padded(cl) if pad else cl, four)


def test_many_big_matches_oracle(shepseg, oracle):
    """289 components of 10100 pixels, each cut once"""
    _check(shepseg, oracle, cs.make('many_big'), True)


def fused_inputs(name):
    """(img, centres, null): one uint8 band cl * 40 + noise(0 .. 11) and the centres 40 c + 6 of the values c >= 1
    of `cl`, so that the noise never moves a pixel to another cluster; where cl is null the band holds the null
    value 255"""
    cl = cs.make(name)
    rng = np.random.RandomState(31)
    img = (cl * 40 + rng.randint(0, 12, size=cl.shape)).astype(np.uint8)
    null = None
    if (cl == 0).any():
        null = 255
        img[cl == 0] = null
    centres = (np.arange(1, int(cl.max()) + 1, dtype=np.float64) * 40 + 6)[:, None]
    return img[None], centres, null


@pytest.mark.parametrize('four', [True, False], ids=['4conn', '8conn'])
@pytest.mark.parametrize('name', ['lattice3', 'strips_h3_mid', 'percolation'])
def test_fused_pipeline_on_cut_shapes(name, four, shepseg, oracle):
    img, centres, null = fused_inputs(name)
    assert np.array_equal(oracle.kmeans_assign(img, centres, null), cs.make(name))
    got = shepseg.doShepherdSegmentation(img, kmeansObj=shepseg.KMeansModel(centres), minSegmentSize=12,
                                         maxSpectralDiff=1e6, imgNullVal=null, fourConnected=four)
    want = oracle.segment_tile(img, centres, 12, 1e6, null, four)
    assert np.array_equal(got.segimg, want['segimg']), _first_difference(got.segimg, want['segimg'])
    assert got.singlePixelsEliminated == want['singlePixelsEliminated']
    assert got.smallSegmentsEliminated == want['smallSegmentsEliminated']
    if name == 'lattice3' and four:
        assert want['singlePixelsEliminated'] >= 2      # the corner pixel and a one-pixel piece of the cut lattice
