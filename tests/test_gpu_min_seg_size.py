"""minSegmentSize across the forms of the small-segment pass loop (elim_small.h k_small_loop).

The loop takes a pass's sources from per-size lists only when min_seg <= 256, 4 * min_seg + 1 <= S + 1
and (S + 1) / min_seg >= 64 (S: segments left after the single-pixel stage); otherwise every pass scans
the whole size table.  Each case below sits on one side of one of those conditions, or past the
depth-first cut's 10000-pixel cap, or past the tile's size, and is compared bit for bit with the oracle."""
import numpy as np
import pytest

from seg_cases import int16_nulls_tile, oracle_tiled, synth_tile

pytestmark = pytest.mark.gpu


def _list_conditions(ms, S):
    return {'ms<=256': ms <= 256, '4ms+1<=S+1': 4 * ms + 1 <= S + 1, 'cap>=64': (S + 1) // ms >= 64}


@pytest.fixture(scope='module')
def shepseg():
    from pyshepseg_amd import shepseg
    return shepseg


_IMG = {}


def _img(oracle, name):
    if name not in _IMG:
        _IMG[name] = {'big': lambda: synth_tile(oracle, 5, 1024, 1024, k=60),
                      'mid': lambda: synth_tile(oracle, 8, 400, 300),
                      'small': lambda: synth_tile(oracle, 9, 200, 150)}[name]()
    return _IMG[name]


# (minSegmentSize, image, which list conditions hold: None = not checked)
CASES = [
    (1, 'mid', None),               # the loop has nothing to do
    (2, 'mid', None),               # size 1 only
    (255, 'big', (True, True, True)),
    (256, 'big', (True, True, True)),       # the list path's upper limit
    (257, 'big', (False, True, True)),      # one above it: the size-table scan
    (100, 'mid', (True, True, False)),      # fails only cap >= 64
    (1000, 'big', (False, True, False)),
    (12000, 'big', (False, False, False)),  # every piece the depth-first cut leaves is small
    (200 * 150 + 7, 'small', (False, False, False)),   # larger than the tile
]


@pytest.mark.parametrize('four', [True, False])
@pytest.mark.parametrize('ms,name,conds', CASES, ids=['%d-%s' % (c[0], c[1]) for c in CASES])
def test_min_seg_size_fused_vs_oracle(ms, name, conds, four, shepseg, oracle):
    img, cen = _img(oracle, name)
    km = shepseg.KMeansModel(cen)
    msd = float(shepseg.autoMaxSpectralDiff(km, 'auto', 50))
    want = oracle.segment_tile(img, cen, ms, msd, None, four)
    S = want['numClumps'] - want['singlePixelsEliminated']
    if conds is not None:
        got = _list_conditions(ms, S)
        assert tuple(got.values()) == conds, (ms, S, got)
    r = shepseg.doShepherdSegmentation(img, kmeansObj=km, minSegmentSize=ms, maxSpectralDiff=msd,
                                       fourConnected=four)
    assert np.array_equal(r.segimg, want['segimg'])
    assert r.singlePixelsEliminated == want['singlePixelsEliminated']
    assert r.smallSegmentsEliminated == want['smallSegmentsEliminated']
    if ms > 200 * 150:
        assert int(r.segimg.max()) == 1 or want['smallSegmentsEliminated'] > 0


@pytest.mark.parametrize('four', [True, False])
def test_min_seg_size_int16_nulls(four, shepseg, oracle):
    img, cen, null = int16_nulls_tile(oracle, 31, 700, 650)
    km = shepseg.KMeansModel(cen)
    msd = float(shepseg.autoMaxSpectralDiff(km, 'auto', 50))
    for ms in (257, 1000):
        want = oracle.segment_tile(img, cen, ms, msd, null, four)
        r = shepseg.doShepherdSegmentation(img, kmeansObj=km, minSegmentSize=ms, maxSpectralDiff=msd,
                                           imgNullVal=null, fourConnected=four)
        assert np.array_equal(r.segimg, want['segimg']), ms
        assert r.smallSegmentsEliminated == want['smallSegmentsEliminated'], ms
        assert (r.segimg[img[0] == null] == 0).all()


@pytest.mark.parametrize('ms', [257, 1000])
def test_min_seg_size_stage_eliminate_small(ms, shepseg, oracle):
    """the stage entry point on the oracle's single-pixel result (same image as the fused cases)"""
    img, cen = _img(oracle, 'big')
    km = shepseg.KMeansModel(cen)
    msd = float(shepseg.autoMaxSpectralDiff(km, 'auto', 50))
    cl = oracle.kmeans_assign(img, cen)
    seg, nxt = oracle.clump(cl, 0, True, 1)
    oracle.eliminate_single_pixels(img, seg, oracle.make_seg_size(seg), 1, nxt - 1, True)
    want = seg.copy()
    ne_want = oracle.eliminate_small_segments(want, img, int(seg.max()), ms, msd, True, 1)
    got = seg.copy()
    ne = shepseg.eliminateSmallSegments(got, img, int(seg.max()), ms, msd, True, 1)
    assert ne == ne_want and np.array_equal(got, want)


@pytest.mark.parametrize('ms', [300, 1000])
def test_min_seg_size_tiled_device_raster(ms, oracle):
    from pyshepseg_amd import tiling
    ras = tiling.DeviceRaster.synth(13, 3, 1100, 1300)
    try:
        img = ras.toArray()
        cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=4)
        r = tiling.doTiledShepherdSegmentation(ras, None, tileSize=512, overlapSize=128, minSegmentSize=ms,
                                               numClusters=30, fixedKMeansInit=True, concurrencyCfg=cfg)
    finally:
        ras.free()
    want, mx, hist = oracle_tiled(oracle, img, r.kmeans.cluster_centers_, 512, 128, ms,
                                  float(r.maxSpectralDiff), None, True)
    assert r.maxSegId == mx
    assert np.array_equal(r.segimg, want)
    assert np.array_equal(r.hist, hist)
