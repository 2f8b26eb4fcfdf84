"""CPU: the numpy definition of the shape table (tests/shape_cases.py) satisfies the perimeter identity against the
neighbour table's definition, shapes.shapeColumnsFromSums gives the closed-form answers on inputs built by hand, its
shift to the bounding box makes the derived columns independent of the origin bit for bit, and calcSegmentShapes
refuses bad arguments before it touches the GPU (there is none here).

Tolerance of the closed forms: numpy.isclose(rtol=1e-12, atol=0).  A dozen float64 operations on small exact integers
stay within tens of ulps of 2.2e-16, so 1e-12 leaves three orders of room."""
import os

import numpy as np
import pytest

import neighbour_cases as nc
import shape_cases as sc
from conftest import GOLDEN


def close(a, b):
    return bool(np.all(np.isclose(a, b, rtol=1e-12, atol=0)))


def derived(counts, sums, missing=-9999):
    from pyshepseg_amd import shapes
    return shapes.shapeColumnsFromSums(counts, sums, missing)


def mosaic():
    with np.load(os.path.join(GOLDEN, 'ci_scenario_1000.npz')) as z:
        return np.ascontiguousarray(z['mosaic'], dtype=np.uint32)


# ---- the model ------------------------------------------------------------------------------------------------------
def test_model_worked_example():
    (counts, sums) = sc.reference_shapes(sc.EXAMPLE)
    for (k, v) in sc.EXAMPLE_COUNTS.items():
        assert counts[k].tolist() == v, k
    for (k, v) in sc.EXAMPLE_SUMS.items():
        assert sums[k].tolist() == v, k


@pytest.mark.parametrize('name', ['mosaic', 'random', 'enclosed'])
def test_model_perimeter_identity(name):
    """perimeter == border length to other segments (4-connected) + outer border, for every id"""
    seg = {'mosaic': mosaic, 'random': lambda: nc.random_labels((64, 96), 40, 1), 'enclosed': nc.enclosed_by_zeros}[name]()
    (counts, _sums) = sc.reference_shapes(seg)
    (offsets, _nbrs, lens) = nc.reference_neighbours(seg, True)
    border = np.zeros(len(offsets) - 1, dtype=np.int64)
    np.add.at(border, np.repeat(np.arange(len(border)), np.diff(offsets)), lens)
    assert np.array_equal(counts['perimeter'], border + counts['outerBorder'])
    assert np.all(counts['edgePixels'] <= counts['area']) and np.all(counts['outerBorder'] <= counts['perimeter'])
    if name == 'enclosed':
        assert counts['perimeter'][3] == counts['outerBorder'][3] == 2 * (10 + 20)


def test_model_variants_agree():
    """the numpy model and the Python-integer model, at the origin and where every sum wraps"""
    seg = nc.random_labels((40, 70), 9, 3)
    for origin in ((0, 0), (2 ** 32 - 40, 2 ** 32 - 70)):
        (c0, s0) = sc.reference_shapes(seg, origin=origin)
        (c1, s1) = sc.reference_shapes_pyint(seg, origin=origin)
        for k in sc.COUNTS:
            assert np.array_equal(c0[k], c1[k]), k
        for k in sc.SUMS:
            assert s0[k].dtype == s1[k].dtype == np.uint64 and np.array_equal(s0[k], s1[k]), k


# ---- shapeColumnsFromSums on hand-built inputs ------------------------------------------------------------------------
def test_single_pixel():
    (counts, sums) = sc.rectangle_sums(1, 1, origin=(7, 9))
    d = derived(counts, sums)
    assert close(d['centroidRow'][1], 7.0) and close(d['centroidCol'][1], 9.0)
    assert close(d['elongation'][1], 1.0)           # both variances 1/12
    assert close(d['compactness'][1], np.pi / 4.0)  # 4 pi 1 / 4^2
    assert close(d['bboxFill'][1], 1.0)
    assert d['orientation'][1] == 0.0               # arctan2(0, 0)


@pytest.mark.parametrize('hw', [(3, 11), (11, 3)])
def test_rectangle(hw):
    """each variance is the side squared over 12, so elongation is max / min"""
    (h, w) = hw
    (counts, sums) = sc.rectangle_sums(h, w)
    assert counts['perimeter'][1] == 2 * h + 2 * w
    d = derived(counts, sums)
    assert close(d['elongation'][1], max(h, w) / min(h, w))
    assert close(d['compactness'][1], 4.0 * np.pi * h * w / (2 * h + 2 * w) ** 2)
    assert close(d['bboxFill'][1], 1.0)
    assert close(d['centroidRow'][1], (h - 1) / 2.0) and close(d['centroidCol'][1], (w - 1) / 2.0)
    if w > h:
        assert d['orientation'][1] == 0.0
    else:
        assert close(d['orientation'][1], np.pi / 2.0)


def test_l_shape():
    """pixels (0,0) (1,0) (2,0) (2,1) (2,2).  By hand: area 5, outline 12; mr = 7/5, mc = 3/5; sum r^2 = 13,
    sum c^2 = 5, sum r c = 6, so vrr = 13/5 - 49/25 + 1/12 = 217/300 = vcc and vrc = 6/5 - 21/25 = 9/25;
    t = 217/150, d = 18/25 = 108/150, lmax = 325/300, lmin = 109/300: elongation sqrt(325/109), and the major axis
    lies on the diagonal towards increasing row, pi/4."""
    seg = np.array([[1, 0, 0], [1, 0, 0], [1, 1, 1]], dtype=np.uint32)
    (counts, sums) = sc.reference_shapes_pyint(seg, 1)
    assert (counts['area'][1], counts['perimeter'][1]) == (5, 12)
    assert [int(sums[k][1]) for k in sc.SUMS] == [7, 3, 13, 5, 6]
    d = derived(counts, sums)
    assert close(d['centroidRow'][1], 7.0 / 5.0) and close(d['centroidCol'][1], 3.0 / 5.0)
    assert close(d['bboxFill'][1], 5.0 / 9.0)
    assert close(d['compactness'][1], 4.0 * np.pi * 5.0 / 144.0)
    assert close(d['elongation'][1], np.sqrt(325.0 / 109.0))
    assert close(d['orientation'][1], np.pi / 4.0)


@pytest.mark.parametrize('hw', [(3, 11), (11, 3)])
def test_origin_near_2_32_changes_no_bit(hw):
    """the sums wrap modulo 2^64 (r^2 alone is just under 2^64 there), the shift to the bounding box undoes it"""
    far = (2 ** 32 - 20, 2 ** 32 - 20)
    (c0, s0) = sc.rectangle_sums(*hw)
    (c1, s1) = sc.rectangle_sums(*hw, origin=far)
    assert int(s1['sumRowRow'][1]) != sum((far[0] + y) ** 2 for y in range(hw[0])) * hw[1]      # it did wrap
    (d0, d1) = (derived(c0, s0), derived(c1, s1))
    for k in ('bboxFill', 'compactness', 'elongation', 'orientation'):
        assert d0[k].tobytes() == d1[k].tobytes(), k
    assert d1['centroidRow'][1] == far[0] + (hw[0] - 1) / 2.0 and d1['centroidCol'][1] == far[1] + (hw[1] - 1) / 2.0


def test_large_segment_far_out_is_exact():
    """a 13 069-pixel segment (a 7 x 1867 band) just below row 2^32: the shifted moments are those at the origin"""
    seg = np.ones((7, 1867), dtype=np.uint32)
    assert seg.size == 13069
    (c0, s0) = sc.reference_shapes(seg, 1)
    (c1, s1) = sc.reference_shapes(seg, 1, origin=(2 ** 32 - 7, 2 ** 32 - 1867))
    (d0, d1) = (derived(c0, s0), derived(c1, s1))
    for k in ('bboxFill', 'compactness', 'elongation', 'orientation'):
        assert d0[k].tobytes() == d1[k].tobytes(), k


def test_rows_without_pixels():
    (counts, sums) = sc.reference_shapes(nc.sparse_ids(), nc.SPARSE_MAX)
    empty = counts['area'] == 0
    assert empty[0] and empty.sum() == nc.SPARSE_MAX + 1 - 3
    for k in sc.COUNTS:
        assert not counts[k][empty].any(), k
    from pyshepseg_amd import shapes
    d = derived(counts, sums, -1234.5)
    assert sorted(d) == sorted(shapes.DERIVED_COLUMNS)
    for k in d:
        assert d[k].dtype == np.float64 and len(d[k]) == nc.SPARSE_MAX + 1
        assert np.all(d[k][empty] == -1234.5) and not np.any(d[k][~empty] == -1234.5), k
    assert np.all(d['elongation'][~empty] >= 1.0)


# ---- refusals, all before the GPU is touched --------------------------------------------------------------------------
SEG = np.ones((4, 5), dtype=np.uint32)
REFUSALS = {
    'float labels': dict(segfile=SEG.astype(np.float32)),
    'int32 labels': dict(segfile=SEG.astype(np.int32)),
    '3-D labels': dict(segfile=np.ones((2, 3, 4), dtype=np.uint32)),
    'no raster': dict(segfile=None),
    'negative maxSegId': dict(segfile=SEG, maxSegId=-1),
    'fractional maxSegId': dict(segfile=SEG, maxSegId=2.5),
    'maxSegId too large': dict(segfile=SEG, maxSegId=0xFFFFFFFE),
    'origin not a pair': dict(segfile=SEG, origin=3),
    'origin of three': dict(segfile=SEG, origin=(1, 2, 3)),
    'negative origin': dict(segfile=SEG, origin=(-1, 0)),
    'fractional origin': dict(segfile=SEG, origin=(0, 1.5)),
    'rows past 2^32': dict(segfile=SEG, origin=(2 ** 32 - 3, 0)),
    'columns past 2^32': dict(segfile=SEG, origin=(0, 2 ** 32 - 4)),
    'chunkPixels 0': dict(segfile=SEG, chunkPixels=0),
    'missingStatsValue': dict(segfile=SEG, missingStatsValue='x'),
}


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_refused_before_the_gpu(name):
    from pyshepseg_amd import shapes
    with pytest.raises(shapes.PyShepSegShapesError):
        shapes.calcSegmentShapes(**REFUSALS[name])


def test_merged_result_without_raster_is_refused():
    from pyshepseg_amd import neighbours, shapes
    with pytest.raises(shapes.PyShepSegShapesError):
        shapes.calcSegmentShapes(neighbours.MergedSegments())
