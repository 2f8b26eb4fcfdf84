"""Host: the model of the junction trace and of the simplification (tests/simplify_cases.py) on the worked example and on
random rasters, what simplifySegmentOutlines refuses before the GPU is touched, and SimplifiedOutlines on results built by
hand."""
import numpy as np
import pytest

import neighbour_cases as nc
import outline_cases as oc
import simplify_cases as sc
from pyshepseg_amd import outlines


def by_hand(m):
    return outlines.SegmentOutlines(m['maxSegId'], m['ringOffsets'], m['vertexOffsets'], m['vertices'], m['ringArea2'],
                                    junction=m['junction'])


# ---- the model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
def test_model_worked_example(four):
    j = sc.reference_junction_trace(oc.EXAMPLE, four)
    plain = oc.reference_outlines(oc.EXAMPLE, four)
    assert len(j['vertices']) == 19 and len(plain['vertices']) == 18
    assert np.array_equal(j['ringArea2'], plain['ringArea2']) and np.array_equal(j['ringOffsets'], plain['ringOffsets'])
    # the one extra vertex: id 3 runs straight through the corner (2, 1), where 1, 2 and 3 meet
    assert j['vertices'][j['vertexOffsets'][2]:].tolist() == [[2, 0], [2, 1], [2, 2], [3, 2], [3, 0]]
    assert j['junction'][j['vertexOffsets'][2]:].tolist() == [1, 1, 0, 1, 0]        # ((2, 2) and (3, 0) have degree 2)
    kept = {}
    for t in sc.TOLERANCES:
        m = sc.reference_simplify(j, t)
        kept[t] = int(m['kept'].sum())
        assert not m['droppedRings'].any() and len(m['vertices']) == kept[t]
    assert kept == {0.0: 19, 0.5: 15, 1.0: 10, 1.5: 9, 4.0: 9}


def test_model_junctions_do_not_depend_on_the_corner_rule_and_saddles_are_junctions():
    deg = sc.corner_degrees(np.array([[1, 2], [2, 1]], dtype=np.uint32))
    assert deg[1, 1] == 4 and deg[0, 1] == 3 and deg[0, 0] == 2
    assert sc.corner_degrees(np.ones((2, 2), dtype=np.uint32))[1, 1] == 0
    # a T-junction on the raster's border: 1 | 2 over the outside
    t = sc.reference_junction_trace(np.array([[1, 2]], dtype=np.uint32))
    assert t['vertices'][t['junction'] == 1].tolist() == [[0, 1], [1, 1], [0, 1], [1, 1]]


@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
def test_model_keeps_one_flag_per_corner(four):
    for seed in range(6):
        seg = nc.random_labels((24, 31), 40, seed)
        j = sc.reference_junction_trace(seg, four)
        plain = oc.reference_outlines(seg, four)
        assert np.array_equal(j['ringArea2'], plain['ringArea2'])
        deg = sc.corner_degrees(seg)
        assert np.array_equal(j['junction'], (deg[j['vertices'][:, 0], j['vertices'][:, 1]] >= 3).astype(np.uint8))
        for t in sc.TOLERANCES:
            m = sc.reference_simplify(j, t)
            assert all(len(f) == 1 for f in sc.corner_flags(j['vertices'], m['kept']).values()), (seed, t)
            assert np.array_equal(m['vertices'], j['vertices'][m['keptVertex']])


def test_model_reversed_arcs_keep_the_mirrored_set():
    T = sc.tolerance2q(1.0)
    (kept, depth) = sc.simplify_arc(sc.TIE_ARC, T)
    assert kept == [True] * 5
    assert sc.simplify_arc(sc.TIE_ARC[::-1], T)[0] == kept[::-1]
    for n in (3, 17, 64, 200):
        for seed in range(3):
            pts = sc.wobble(n, seed)
            for t in sc.TOLERANCES:
                (a, da) = sc.simplify_arc(pts, sc.tolerance2q(t))
                (b, db) = sc.simplify_arc(pts[::-1], sc.tolerance2q(t))
                assert a == b[::-1] and da == db, (n, seed, t)
    for n in (8, 65, 300):
        assert sc.simplify_arc(sc.zigzag(n), sc.tolerance2q(0.5))[1] == n - 2


def test_model_on_the_boundary_of_the_tolerance():
    """the point (1, 1) over the chord (0, 0) - (0, 2): m = 2, |b - a|^2 = 4, so it exceeds when 4 * 65536 > 4 T"""
    arc = [(0, 0), (1, 1), (0, 2)]
    assert sc.tolerance2q(1.0) == 65536
    assert sc.simplify_arc(arc, 65536)[0] == [True, False, True] and sc.simplify_arc(arc, 65535)[0] == [True, True, True]


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_everything_refusable_is_refused_before_the_gpu_is_touched(monkeypatch):
    from pyshepseg_amd import _lib

    def no_gpu():
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(_lib, 'ctx', no_gpu)
    monkeypatch.setattr(_lib, 'lib', no_gpu)
    E = outlines.PyShepSegOutlinesError
    m = sc.reference_junction_trace(oc.EXAMPLE)
    plain = outlines.SegmentOutlines(3, m['ringOffsets'], m['vertexOffsets'], m['vertices'], m['ringArea2'])
    assert plain.junction is None and plain.simplified is None
    with pytest.raises(E, match='junctions=True'):
        outlines.simplifySegmentOutlines(plain, 1.0)
    o = by_hand(m)
    for tol in (-0.5, float('nan'), 32768.5, float('inf'), 'wide', None, True):
        with pytest.raises(E, match='tolerance must be a number 0 .. 32768'):
            outlines.simplifySegmentOutlines(o, tol)
        with pytest.raises(E, match='tolerance must be a number 0 .. 32768'):
            outlines.traceSegmentOutlines(oc.EXAMPLE, simplify=tol) if tol is not None else outlines.tolerance2q(tol)
    for flags in (m['junction'].astype(np.int32), m['junction'][:-1], m['junction'].reshape(1, -1), m['junction'].astype(bool)):
        o.junction = flags
        with pytest.raises(E, match='junction must be a uint8 array with one entry per vertex'):
            outlines.simplifySegmentOutlines(o, 1.0)
    wide = sc.outlines_from({1: [([(0, 0), (0, 2 ** 16 + 1), (2 ** 16, 2 ** 16 + 1), (2 ** 16, 0)], [1, 0, 0, 0])]})
    with pytest.raises(E, match='span 65536 rows and 65537 columns'):
        outlines.simplifySegmentOutlines(by_hand(wide), 1.0)
    long = sc.outlines_from({1: [([(0, 0), (0, 1), (2 ** 31, 1), (2 ** 31, 0)], [1, 0, 0, 0])]})
    with pytest.raises(E, match='span 2147483648 rows'):
        outlines.simplifySegmentOutlines(by_hand(long), 1.0)
    for path in ('fast', 'AUTO', 2, None):
        with pytest.raises(E, match="path must be one of 'auto', 'short', 'group', 'global'"):
            outlines.simplifySegmentOutlines(by_hand(m), 1.0, path=path)
    assert outlines.tolerance2q(0) == 0 and outlines.tolerance2q(0.5) == 16384 and outlines.tolerance2q(32768) == 2 ** 46
    for t in (0.3, 1.0 / 3.0, 1.5, 4.0, 1234.5678):
        assert outlines.tolerance2q(t) == sc.tolerance2q(t)
    # the call itself does reach for the GPU once its arguments stand
    with pytest.raises(AssertionError, match='the GPU was touched'):
        outlines.simplifySegmentOutlines(by_hand(m), 1.0)


# ---- results built by hand ---------------------------------------------------------------------------------------------
def shell(a, b):
    return [(a, a), (a, b), (b, b), (b, a)]


def hole(a, b):
    return [(a, b), (a, a), (b, a), (b, b)]


def source_by_hand():
    """id 1: two shells side by side (the second moved 20 columns), a hole in each"""
    def moved(r):
        return [(y, x + 20) for (y, x) in r]
    rings = [shell(0, 10), hole(2, 8), moved(shell(0, 10)), moved(hole(2, 8))]
    verts = np.array([v for r in rings for v in r], dtype=np.int64)
    return outlines.SegmentOutlines(1, np.array([0, 0, 4], dtype=np.int64), np.arange(0, 17, 4, dtype=np.int64), verts,
                                    np.array([oc.area2(r) for r in rings], dtype=np.int64),
                                    junction=np.zeros(16, dtype=np.uint8))


def simplified_by_hand(src, rings):
    """rings: (source ring, [kept positions in it]); slanted where a corner is left out"""
    kv = np.array([int(src.vertexOffsets[r]) + i for (r, idx) in rings for i in idx], dtype=np.int64)
    vo = np.concatenate([[0], np.cumsum([len(idx) for (_r, idx) in rings])]).astype(np.int64)
    verts = src.vertices[kv]
    area = np.array([oc.area2(verts[vo[k]:vo[k + 1]].tolist()) for k in range(len(rings))], dtype=np.int64)
    return outlines.SimplifiedOutlines(src, np.array([0, 0, len(rings)], dtype=np.int64), vo, verts, area,
                                       np.array([r for (r, _idx) in rings], dtype=np.int64), kv, tolerance=3.0,
                                       tolerance2q=outlines.tolerance2q(3.0))


def test_simplified_polygons_follow_the_source():
    src = source_by_hand()
    assert [len(p) for p in src.polygonsOf(1)] == [2, 2]
    # triangles: every ring loses its last corner, so all of them are slanted; the holes follow their source shells
    s = simplified_by_hand(src, [(0, [0, 1, 2]), (1, [0, 1, 2]), (2, [0, 1, 2]), (3, [0, 1, 2])])
    assert isinstance(s, outlines.SegmentOutlines) and s.source is src and s.residentSerial is None
    assert s.ringArea2.tolist() == [100, -36, 100, -36] and s.droppedRings.tolist() == [0, 0]
    assert s.columns['droppedRings'] is s.droppedRings and s.columns['numParts'].tolist() == [0, 2]
    assert s.columns['numVertices'].tolist() == [0, 12] and s.junction.dtype == np.uint8 and len(s.junction) == 12
    polys = [[r.tolist() for r in poly] for poly in s.polygonsOf(1)]
    assert polys == [[[[0, 0], [0, 10], [10, 10]], [[2, 8], [2, 2], [8, 2]]],
                     [[[0, 20], [0, 30], [10, 30]], [[2, 28], [2, 22], [8, 22]]]]
    # the first shell dropped: its hole is left out, the other polygon stays whole
    s = simplified_by_hand(src, [(1, [0, 1, 2]), (2, [0, 1, 2, 3]), (3, [0, 1, 2])])
    assert s.droppedRings.tolist() == [0, 1] and s.sourceRing.tolist() == [1, 2, 3]
    polys = [[r.tolist() for r in poly] for poly in s.polygonsOf(1)]
    assert polys == [[[[0, 20], [0, 30], [10, 30], [10, 20]], [[2, 28], [2, 22], [8, 22]]]]
    assert outlines.toWKT(s, 1) == 'MULTIPOLYGON (((20 0, 30 0, 30 10, 20 10, 20 0), (28 2, 22 2, 22 8, 28 2)))'
    assert outlines.toWKT(s, 0) == 'MULTIPOLYGON EMPTY'
    with pytest.raises(outlines.PyShepSegOutlinesError, match='segment id'):
        s.polygonsOf(2)


def test_simplified_geojson(tmp_path):
    import json
    src = source_by_hand()
    s = simplified_by_hand(src, [(0, [0, 1, 2]), (1, [0, 1, 2]), (2, [0, 1, 2]), (3, [0, 1, 2])])
    path = str(tmp_path / 's.geojson')
    assert outlines.writeGeoJSON(s, path, columns={'droppedRings': s.droppedRings}) == 1
    with open(path) as f:
        g = json.load(f)
    coords = g['features'][0]['geometry']['coordinates']
    assert [len(poly) for poly in coords] == [2, 2] and coords[0][0][0] == coords[0][0][-1] and len(coords[0][0]) == 4


def test_a_segment_outlines_built_by_hand_can_carry_flags():
    m = sc.reference_junction_trace(oc.EXAMPLE)
    o = by_hand(m)
    assert o.junction is m['junction'] and o.hulls is None and o.simplified is None
    assert outlines.SegmentOutlines(3, m['ringOffsets'], m['vertexOffsets'], m['vertices'], m['ringArea2']).junction is None
