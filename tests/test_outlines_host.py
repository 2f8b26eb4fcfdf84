"""CPU: the sequential model of segment outlines (tests/outline_cases.py) on the worked examples and its identities on
random rasters; the host side of pyshepseg_amd.outlines -- polygonsOf, toWKT, writeGeoJSON, the argument refusals -- on
hand-built SegmentOutlines.  Nothing here touches a GPU."""
import json

import numpy as np
import pytest

import outline_cases as oc
import shape_cases as sc
from pyshepseg_amd import outlines


def built(seg, fourConnected=True, maxSegId=None, origin=(0, 0)):
    """a SegmentOutlines from the model's arrays"""
    m = oc.reference_outlines(seg, fourConnected, maxSegId, origin)
    return outlines.SegmentOutlines(m['maxSegId'], m['ringOffsets'], m['vertexOffsets'], m['vertices'], m['ringArea2'],
                                    origin=origin, fourConnected=fourConnected)


# ---- the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('four', [True, False])
def test_model_worked_example(four):
    m = oc.reference_outlines(oc.EXAMPLE, four)
    assert m['ringOffsets'].tolist() == [0, 0, 1, 2, 3] and m['vertexOffsets'].tolist() == [0, 6, 14, 18]
    assert m['ringArea2'].tolist() == oc.EXAMPLE_AREA2
    want = [v for i in (1, 2, 3) for ring in oc.EXAMPLE_RINGS[i] for v in ring]
    assert m['vertices'].tolist() == [list(v) for v in want]
    assert all(m[k].dtype == np.int64 for k in ('ringOffsets', 'vertexOffsets', 'vertices', 'ringArea2'))


def test_model_checkerboard():
    four = oc.reference_outlines(oc.checkerboard(4), True)
    assert len(four['ringArea2']) == 8 and np.diff(four['vertexOffsets']).tolist() == [4] * 8
    assert four['ringArea2'].tolist() == [2] * 8
    eight = oc.reference_outlines(oc.checkerboard(4), False)
    assert list(zip(eight['ringArea2'].tolist(), np.diff(eight['vertexOffsets']).tolist())) == [(20, 24), (-2, 4), (-2, 4)]
    assert eight['columns']['numParts'].tolist() == [0, 1] and eight['columns']['numHoles'].tolist() == [0, 2]
    assert eight['columns']['holeArea'].tolist() == [0, 2] and eight['columns']['numVertices'].tolist() == [0, 32]


def check_identities(seg, m, four):
    (counts, _sums) = sc.reference_shapes(seg, m['maxSegId'])
    ro = m['ringOffsets']
    a2 = np.concatenate([[0], np.cumsum(m['ringArea2'])])
    assert np.array_equal(a2[ro[1:]] - a2[ro[:-1]], 2 * counts['area'])
    ln = np.concatenate([[0], np.cumsum(oc.ring_lengths(m['vertexOffsets'], m['vertices']))])
    assert np.array_equal(ln[ro[1:]] - ln[ro[:-1]], counts['perimeter'])
    assert np.array_equal(oc.ring_lengths(m['vertexOffsets'], m['vertices']), m['ringEdges'])
    has = np.flatnonzero(np.diff(ro) > 0)
    assert np.all(m['ringArea2'][ro[has]] > 0)
    assert np.array_equal(oc.rasterise(seg.shape, ro, m['vertexOffsets'], m['vertices']), seg)
    nv = np.diff(m['vertexOffsets'])
    assert np.all(nv >= 4) and not np.any(nv & 1)


@pytest.mark.parametrize('four', [True, False])
def test_model_identities_on_random_rasters(four):
    """(walk_rings itself asserts that every walk closes on its first edge and that the rings cover every edge once:
    the successor map is a permutation)"""
    for seed in range(30):
        rng = np.random.default_rng(seed)
        shape = (int(rng.integers(1, 20)), int(rng.integers(1, 20)))
        seg = oc.random_labels(shape, int(rng.integers(1, 5)), 100 + seed)
        check_identities(seg, oc.reference_outlines(seg, four), four)
    seg = oc.concentric_squares()
    check_identities(seg, oc.reference_outlines(seg, four), four)


def test_model_leader_is_a_turn_edge_not_the_smallest_edge():
    """the smallest edge of a hole three pixels wide is S of (0, 1), whose predecessor S of (0, 2) has the same side: the
    ring begins at S of (0, 3), its smallest TURN edge"""
    seg = np.ones((4, 5), dtype=np.uint32)
    seg[1:3, 1:4] = 0
    m = oc.reference_outlines(seg, True)
    assert m['ringArea2'].tolist() == [40, -12]
    ring = m['vertices'][m['vertexOffsets'][1]:m['vertexOffsets'][2]].tolist()
    assert ring == [[1, 4], [1, 1], [3, 1], [3, 4]]


# ---- polygons ------------------------------------------------------------------------------------------------------
def shell(a, b):
    return [(a, a), (a, b), (b, b), (b, a)]


def hole(a, b):
    return [(a, b), (a, a), (b, a), (b, b)]


def squares_by_hand():
    """concentric squares of the ids 1, 2, 1, 2, 1, two pixels wide, in 18 x 18: square k spans [2 k, 18 - 2 k)"""
    rings1 = [shell(0, 18), hole(2, 16), shell(4, 14), hole(6, 12), shell(8, 10)]
    rings2 = [shell(2, 16), hole(4, 14), shell(6, 12), hole(8, 10)]
    rings = rings1 + rings2
    verts = np.array([v for r in rings for v in r], dtype=np.int64)
    vo = np.arange(0, 4 * len(rings) + 1, 4, dtype=np.int64)
    area2 = np.array([oc.area2(r) for r in rings], dtype=np.int64)
    ro = np.array([0, 0, 5, 9], dtype=np.int64)
    return outlines.SegmentOutlines(2, ro, vo, verts, area2)


def test_polygons_of_concentric_squares():
    o = squares_by_hand()
    m = oc.reference_outlines(oc.concentric_squares())
    for k in ('ringOffsets', 'vertexOffsets', 'vertices', 'ringArea2'):
        assert np.array_equal(getattr(o, k), m[k]), k
    assert o.ringArea2.tolist() == [648, -392, 200, -72, 8, 392, -200, 72, -8]
    assert {k: v.tolist() for (k, v) in o.columns.items()} == {
        'numParts': [0, 3, 2], 'numHoles': [0, 2, 2], 'numVertices': [0, 20, 16], 'holeArea': [0, 232, 104]}
    for k in oc.COLUMNS:
        assert o.columns[k].dtype == np.int64 and np.array_equal(o.columns[k], m['columns'][k])
    p1 = [[r.tolist() for r in poly] for poly in o.polygonsOf(1)]
    assert p1 == [[[list(v) for v in shell(0, 18)], [list(v) for v in hole(2, 16)]],
                  [[list(v) for v in shell(4, 14)], [list(v) for v in hole(6, 12)]],
                  [[list(v) for v in shell(8, 10)]]]
    p2 = [[r.tolist() for r in poly] for poly in o.polygonsOf(2)]
    assert p2 == [[[list(v) for v in shell(2, 16)], [list(v) for v in hole(4, 14)]],
                  [[list(v) for v in shell(6, 12)], [list(v) for v in hole(8, 10)]]]
    assert o.polygonsOf(0) == [] and o.ringsOf(0) == [] and len(o.ringsOf(1)) == 5
    with pytest.raises(outlines.PyShepSegOutlinesError, match='segment id'):
        o.ringsOf(3)


def test_polygons_with_an_origin_and_holes_beside_each_other():
    """two shells of one id side by side, a hole in each; the origin moves shells and holes alike"""
    seg = np.zeros((7, 12), dtype=np.uint32)
    seg[0:5, 0:5] = 1
    seg[1:6, 6:12] = 1
    seg[2, 2] = 0
    seg[3, 9] = 2
    o = built(seg, origin=(100, 1000))
    polys = o.polygonsOf(1)
    assert [len(p) for p in polys] == [2, 2]
    assert polys[0][1].tolist() == [[103, 1003], [103, 1002], [102, 1002], [102, 1003]] or \
        polys[0][1].tolist() == [[102, 1003], [102, 1002], [103, 1002], [103, 1003]]
    assert polys[1][1][:, 1].min() == 1009 and polys[1][1][:, 0].min() == 103


# ---- WKT and GeoJSON -----------------------------------------------------------------------------------------------
def test_wkt():
    o = built(oc.EXAMPLE)
    assert outlines.toWKT(o, 3) == 'MULTIPOLYGON (((0 2, 2 2, 2 3, 0 3, 0 2)))'
    assert outlines.toWKT(o, 0) == 'MULTIPOLYGON EMPTY'
    t = (500000.0, 10.0, 0.0, 7000000.0, 0.0, -10.0)
    assert outlines.toWKT(o, 3, transform=t) == \
        'MULTIPOLYGON (((500000 6999980, 500020 6999980, 500020 6999970, 500000 6999970, 500000 6999980)))'
    sq = squares_by_hand()
    wkt = outlines.toWKT(sq, 2)
    assert wkt == ('MULTIPOLYGON (((2 2, 16 2, 16 16, 2 16, 2 2), (14 4, 4 4, 4 14, 14 14, 14 4)), '
                   '((6 6, 12 6, 12 12, 6 12, 6 6), (10 8, 8 8, 8 10, 10 10, 10 8)))')
    with pytest.raises(outlines.PyShepSegOutlinesError, match='six'):
        outlines.toWKT(o, 3, transform=(0, 1, 0))


def test_geojson(tmp_path):
    o = squares_by_hand()
    path = str(tmp_path / 'a.geojson')
    assert outlines.writeGeoJSON(o, path) == 2
    with open(path) as f:
        doc = json.load(f)
    assert doc['type'] == 'FeatureCollection' and [ft['properties'] for ft in doc['features']] == [{'segId': 1}, {'segId': 2}]
    g = doc['features'][0]['geometry']
    assert g['type'] == 'MultiPolygon' and [len(p) for p in g['coordinates']] == [2, 2, 1]
    assert g['coordinates'][2][0] == [[8, 8], [10, 8], [10, 10], [8, 10], [8, 8]]
    # chosen ids, a transform and columns
    t = (100.0, 2.0, 0.0, 50.0, 0.0, -2.0)
    cols = dict(o.columns)
    cols['mean'] = np.array([0.0, 1.5, 2.5])
    cols['name'] = ['none', 'a', 'b']
    path = str(tmp_path / 'b.geojson')
    assert outlines.writeGeoJSON(o, path, ids=[2], transform=t, columns=cols) == 1
    with open(path) as f:
        doc = json.load(f)
    (ft,) = doc['features']
    assert ft['properties'] == {'segId': 2, 'numParts': 2, 'numHoles': 2, 'numVertices': 16, 'holeArea': 104, 'mean': 2.5,
                                'name': 'b'}
    assert ft['geometry']['coordinates'][0][0] == [[104, 46], [132, 46], [132, 18], [104, 18], [104, 46]]
    with pytest.raises(outlines.PyShepSegOutlinesError, match='rows'):
        outlines.writeGeoJSON(o, path, columns={'short': np.zeros(2)})
    # an id without pixels is a feature without polygons
    assert outlines.writeGeoJSON(o, path, ids=[0]) == 1
    with open(path) as f:
        assert json.load(f)['features'][0]['geometry'] == {'type': 'MultiPolygon', 'coordinates': []}


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_arguments_are_refused_before_the_gpu_is_touched(monkeypatch):
    from pyshepseg_amd import _lib, neighbours

    def no_gpu():
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(_lib, 'ctx', no_gpu)
    E = outlines.PyShepSegOutlinesError
    seg = oc.EXAMPLE
    with pytest.raises(E, match='2-D uint32'):
        outlines.traceSegmentOutlines(seg.astype(np.int32))
    with pytest.raises(E, match='2-D uint32'):
        outlines.traceSegmentOutlines(seg.ravel())
    with pytest.raises(E, match='maxSegId must be a non-negative integer'):
        outlines.traceSegmentOutlines(seg, maxSegId=-1)
    with pytest.raises(E, match='too large'):
        outlines.traceSegmentOutlines(seg, maxSegId=2 ** 32 - 1)
    for origin in (5, (1, 2, 3), (-1, 0), (0.5, 0), (True, 0)):
        with pytest.raises(E, match='origin'):
            outlines.traceSegmentOutlines(seg, origin=origin)
    with pytest.raises(E, match='past coordinate'):
        outlines.traceSegmentOutlines(seg, origin=(2 ** 32 - 2, 0))
    m = neighbours.MergedSegments.__new__(neighbours.MergedSegments)
    m.outDev = None
    m.segimg = None
    m.maxSegId = 3
    with pytest.raises(E, match='no recoded raster'):
        outlines.traceSegmentOutlines(m)
    # the call itself does reach for the GPU once its arguments stand
    with pytest.raises(AssertionError, match='the GPU was touched'):
        outlines.traceSegmentOutlines(seg)
