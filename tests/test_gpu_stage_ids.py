"""The stage entry points' id arguments against the oracle: clump's clumpId and ignoreVal, and the
minSegId of eliminateSinglePixels / eliminateSmallSegments (reference shepseg.py:964 starts the
elimination's id range at it; relabelSegments, :766-769, keeps the ids up to it and closes the gaps
above it).  Ids that start at minSegId, above it, and below it."""
import numpy as np
import pytest

from seg_cases import synth_tile

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def shepseg():
    from pyshepseg_amd import shepseg
    return shepseg


@pytest.fixture(scope='module')
def tile(oracle):
    img, cen = synth_tile(oracle, 17, 300, 340, k=40)
    return img, cen, oracle.kmeans_assign(img, cen)


@pytest.mark.parametrize('four', [True, False])
@pytest.mark.parametrize('ignore,clump_id', [(0, 7), (3, 1), (5, 1000)])
def test_clump_ids_and_ignore_value(ignore, clump_id, four, tile, shepseg, oracle):
    cl = tile[2].astype(np.int32)
    assert ignore == 0 or (cl == ignore).any()
    seg, nxt = shepseg.clump(cl, ignore, fourConnected=four, clumpId=clump_id)
    oseg, onxt = oracle.clump(cl, ignore, four, clump_id)
    assert nxt == onxt and np.array_equal(seg, oseg)
    assert (seg[cl == ignore] == 0).all() and int(seg[seg != 0].min()) == clump_id


def _shifted(seg, first):
    """seg with its ids moved to start at `first` (null stays 0)"""
    out = seg.copy()
    out[out != 0] += np.uint32(first - 1)
    return out


# (first id of the input, minSegId)
IDS = [(5, 5), (9, 5), (1, 40), (1, 1)]


@pytest.mark.parametrize('first,min_id', IDS)
def test_eliminate_single_pixels_min_seg_id(first, min_id, tile, shepseg, oracle):
    img, cen, cl = tile
    seg0, nxt = oracle.clump(cl, 0, True, 1)
    seg = _shifted(seg0, first)
    mx = int(seg.max())
    want = seg.copy()
    oracle.eliminate_single_pixels(img, want, oracle.make_seg_size(want), min_id, mx, True)
    got = seg.copy()
    shepseg.eliminateSinglePixels(img, got, shepseg.makeSegSize(got), min_id, mx, True)
    assert np.array_equal(got, want)
    if first < min_id:           # ids below minSegId keep their number, gaps among them stay
        assert not np.array_equal(got, oracle_relabel_from_one(oracle, img, seg, mx))


def oracle_relabel_from_one(oracle, img, seg, mx):
    out = seg.copy()
    oracle.eliminate_single_pixels(img, out, oracle.make_seg_size(out), 1, mx, True)
    return out


@pytest.mark.parametrize('four', [True, False])
@pytest.mark.parametrize('first,min_id', IDS)
def test_eliminate_small_segments_min_seg_id(first, min_id, four, tile, shepseg, oracle):
    img, cen, cl = tile
    seg0, nxt = oracle.clump(cl, 0, four, 1)
    oracle.eliminate_single_pixels(img, seg0, oracle.make_seg_size(seg0), 1, nxt - 1, four)
    seg = _shifted(seg0, first)
    mx = int(seg.max())
    msd = float(shepseg.autoMaxSpectralDiff(shepseg.KMeansModel(cen), 'auto', 50))
    for ms in (20, 300):
        want = seg.copy()
        ne_want = oracle.eliminate_small_segments(want, img, mx, ms, msd, four, min_id)
        got = seg.copy()
        ne = shepseg.eliminateSmallSegments(got, img, mx, ms, msd, four, min_id)
        assert ne == ne_want and np.array_equal(got, want), (ms, first, min_id)
        if first < min_id:
            # segments below minSegId are never sources: some small ones are left that minSegId 1 merges
            small_left = np.bincount(got.ravel())[1:min_id]
            assert ((small_left > 0) & (small_left < ms)).any()


def test_min_seg_id_zero_is_refused(tile, shepseg):
    img, cen, cl = tile
    seg = np.ones(cl.shape, dtype=np.uint32)
    with pytest.raises(ValueError):
        shepseg.eliminateSinglePixels(img, seg, shepseg.makeSegSize(seg), 0, 1, True)
    with pytest.raises(ValueError):
        shepseg.eliminateSmallSegments(seg, img, 1, 10, 1e9, True, 0)
