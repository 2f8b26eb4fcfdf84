"""CPU: the sequential model of segment hulls (tests/hull_cases.py) against the definition of an extreme point; the host
side of the hulls in pyshepseg_amd.outlines -- hullColumnsFromSums on hand values, the limits calcSegmentHulls checks
before it touches the GPU, hullOf's id check, the ``missing`` fill.  Nothing here touches a GPU."""
import math

import numpy as np
import pytest

import hull_cases as hc
import neighbour_cases as nc
import outline_cases as oc
from pyshepseg_amd import outlines


def built(seg, fourConnected=True, maxSegId=None, origin=(0, 0)):
    m = oc.reference_outlines(seg, fourConnected, maxSegId, origin)
    return outlines.SegmentOutlines(m['maxSegId'], m['ringOffsets'], m['vertexOffsets'], m['vertices'], m['ringArea2'],
                                    origin=origin, fourConnected=fourConnected)


def host_columns(o, missing=-9999):
    """hullColumnsFromSums fed with the model's integers"""
    m = hc.reference_hulls(o, missing)
    a2 = outlines._segmentSums(o.ringArea2, o.ringOffsets)
    per = outlines._segmentSums(oc.ring_lengths(o.vertexOffsets, o.vertices), o.ringOffsets)
    return (m, outlines.hullColumnsFromSums(m['sums'], m['hullOffsets'], m['hullPoints'], m['hullReach'], a2, per, missing))


# ---- the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('four', [True, False])
def test_model_against_the_definition_of_an_extreme_point(four):
    for seed in range(6):
        seg = nc.random_labels((6, 7), 3, 50 + seed)
        o = built(seg, four)
        m = hc.reference_hulls(o)
        for i in range(o.maxSegId + 1):
            h = m['hullPoints'][m['hullOffsets'][i]:m['hullOffsets'][i + 1]]
            verts = [tuple(p) for ring in o.ringsOf(i) for p in ring.tolist()]
            assert set(map(tuple, h.tolist())) == hc.extreme_points(verts)
            assert len(h) == len(set(map(tuple, h.tolist())))
            if len(h):
                assert oc.area2(h) > 0 and tuple(h[0]) == min(map(tuple, h.tolist()))
                nxt = np.roll(h, -1, axis=0)
                nn = np.roll(h, -2, axis=0)
                turn = (nxt[:, 1] - h[:, 1]) * (nn[:, 0] - h[:, 0]) - (nxt[:, 0] - h[:, 0]) * (nn[:, 1] - h[:, 1])
                assert np.all(turn > 0)


def test_model_worked_hulls():
    m = hc.reference_hulls(built(hc.L_SHAPE))
    assert m['hullPoints'].tolist() == [[0, 0], [0, 1], [2, 3], [3, 3], [3, 0]]
    assert m['sums']['hullArea2'].tolist() == [0, 14] and m['sums']['feretMax2'].tolist() == [0, 18]
    m = hc.reference_hulls(built(hc.PLUS))
    assert m['hullPoints'].tolist() == [[0, 1], [0, 2], [1, 3], [2, 3], [3, 2], [3, 1], [2, 0], [1, 0]]
    assert m['sums']['hullArea2'].tolist() == [0, 14] and m['sums']['feretMax2'].tolist() == [0, 10]
    assert m['hullReach'].tolist() == [3, 4, 3, 4, 3, 4, 3, 4]


# ---- the derived columns ------------------------------------------------------------------------------------------
def test_one_pixel():
    (m, cols) = host_columns(built(np.ones((1, 1), dtype=np.uint32)))
    assert m['sums']['hullArea2'][1] == 2 and m['sums']['feretMax2'][1] == 2 and m['sums']['numHullVertices'][1] == 4
    assert cols['feretMin'][1] == 1.0 and cols['solidity'][1] == 1.0 and cols['hullArea'][1] == 1.0
    assert cols['feretMax'][1] == math.sqrt(2.0) and cols['convexity'][1] == 1.0 and cols['hullPerimeter'][1] == 4.0
    assert sorted(cols) == sorted(outlines.HULL_DERIVED) and all(c.dtype == np.float64 for c in cols.values())


@pytest.mark.parametrize('ab', [(1, 9), (9, 1), (3, 5), (40, 7)])
def test_rectangles(ab):
    (a, b) = ab
    (m, cols) = host_columns(built(np.ones((a, b), dtype=np.uint32), origin=(5, 3)))
    assert m['hullPoints'].tolist() == [[5, 3], [5, 3 + b], [5 + a, 3 + b], [5 + a, 3]]
    assert cols['solidity'][1] == 1.0 and cols['feretMin'][1] == float(min(a, b))
    assert m['sums']['feretMax2'][1] == a * a + b * b and cols['feretMax'][1] == math.sqrt(a * a + b * b)
    assert cols['feretRatio'][1] == min(a, b) / math.sqrt(a * a + b * b) and cols['convexity'][1] == 1.0


def test_l_shape_and_plus_sign():
    (_m, cols) = host_columns(built(hc.L_SHAPE))
    assert cols['hullArea'][1] == 7.0 and cols['solidity'][1] == 5.0 / 7.0
    assert cols['hullPerimeter'][1] == pytest.approx(1 + math.sqrt(8) + 1 + 3 + 3, rel=1e-15)
    assert cols['convexity'][1] == pytest.approx((8 + math.sqrt(8)) / 12.0, rel=1e-15)
    # the narrowest pair of support lines lies along the diagonal edge (0, 1) -> (2, 3), with (3, 0) opposite: 8 / sqrt(8)
    assert cols['feretMax'][1] == math.sqrt(18) and cols['feretMin'][1] == pytest.approx(math.sqrt(8), rel=1e-15)
    (_m, cols) = host_columns(built(hc.PLUS))
    assert cols['hullArea'][1] == 7.0 and cols['solidity'][1] == 5.0 / 7.0
    assert cols['hullPerimeter'][1] == pytest.approx(4 + 4 * math.sqrt(2), rel=1e-15)
    # across the diagonal edges the octagon is 4 / sqrt(2) wide, less than the 3 across the straight ones
    assert cols['feretMin'][1] == pytest.approx(math.sqrt(8), rel=1e-15) and cols['feretMax'][1] == math.sqrt(10)


def test_host_columns_agree_with_the_model_and_missing_fills():
    seg = nc.random_labels((20, 30), 9, 4)
    seg[seg == 4] = 0
    o = built(seg, maxSegId=12)
    (m, cols) = host_columns(o, missing=-1.5)
    none = [0, 4, 10, 11, 12]
    for name in outlines.HULL_DERIVED:
        assert np.allclose(cols[name], m['columns'][name], rtol=1e-12, atol=0), name
        assert np.all(cols[name][none] == -1.5) and not np.any(np.delete(cols[name], none) == -1.5), name
    assert np.all((cols['solidity'][1:4] > 0) & (cols['solidity'][1:4] <= 1))
    assert not m['sums']['numHullVertices'][none].any()


# ---- what is refused before the GPU is touched --------------------------------------------------------------------
def test_limits_are_checked_on_the_host(monkeypatch):
    from pyshepseg_amd import _lib

    def no_gpu():
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(_lib, 'ctx', no_gpu)
    wide = hc.outlines_from_rings({1: [hc.rectangle_ring(0, 0, 2 ** 16 + 1, 2 ** 16)]})
    with pytest.raises(outlines.PyShepSegOutlinesError, match='span 65537 rows and 65536 columns'):
        outlines.calcSegmentHulls(wide)
    tall = hc.outlines_from_rings({1: [hc.rectangle_ring(7, 7, 2 ** 31, 1)]})
    with pytest.raises(outlines.PyShepSegOutlinesError, match='max\\(H, W\\) < 2\\^31'):
        outlines.calcSegmentHulls(tall)
    ok = hc.outlines_from_rings({1: [hc.rectangle_ring(0, 0, 2 ** 31 - 1, 2)]})
    with pytest.raises(AssertionError, match='the GPU was touched'):
        outlines.calcSegmentHulls(ok)                   # within the limits: the next step is the context
    o = built(oc.EXAMPLE)
    o.vertexOffsets = o.vertexOffsets[::-1].copy()
    with pytest.raises(outlines.PyShepSegOutlinesError, match='vertexOffsets must ascend'):
        outlines.calcSegmentHulls(o)
    o = built(oc.EXAMPLE)
    o.vertices = o.vertices.astype(np.int32)
    with pytest.raises(outlines.PyShepSegOutlinesError, match='vertices must be an int64 array'):
        outlines.calcSegmentHulls(o)
    o = built(oc.EXAMPLE)
    o.maxSegId = 7
    with pytest.raises(outlines.PyShepSegOutlinesError, match='maxSegId \\+ 2 entries'):
        outlines.calcSegmentHulls(o)


def test_hull_of_checks_the_id():
    m = hc.reference_hulls(built(oc.EXAMPLE))
    h = outlines.SegmentHulls(m['maxSegId'], m['hullOffsets'], m['hullPoints'], m['hullReach'], m['sums'], m['columns'])
    assert h.hullOf(0).shape == (0, 2) and h.hullOf(3).tolist() == [[2, 0], [2, 2], [3, 2], [3, 0]]
    assert h.hullOf(np.int64(1)).base is not None
    for bad in (-1, 4, 1.0, True, '1', None):
        with pytest.raises(outlines.PyShepSegOutlinesError, match='segment id must be an integer 0 .. 3'):
            h.hullOf(bad)
