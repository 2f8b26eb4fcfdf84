"""GPU: the junction trace and outlines.simplifySegmentOutlines against the sequential model in Python integers
(tests/simplify_cases.py): numpy.array_equal on every integer array, dtype included.

The kernels (csrc/simplify.h) take a vertex, an arc, a point, a ring or an id per thread in workgroups of 256; an arc is
simplified by one of three classes by its point count: up to SP_SHORT_MAX = 64 by one wavefront, up to SP_GROUP_MAX =
1024 by one workgroup (both with the points in LDS and the round loop in the kernel), beyond that in global arrays with
the rounds launched from the host.  The `path` argument forces a class for all arcs that fit it, so every class is
reached at small sizes; the shared scan takes 8192 items a workgroup."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import neighbour_cases as nc
import outline_cases as oc
import simplify_cases as sc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RINGS = ('ringOffsets', 'vertexOffsets', 'vertices', 'ringArea2')
RESULT = RINGS + ('sourceRing', 'keptVertex', 'droppedRings', 'junction')
PATHS = ('auto', 'short', 'group', 'global')


def trace(seg, **kw):
    from pyshepseg_amd import outlines
    return outlines.traceSegmentOutlines(seg, **kw)


def simplify(o, tolerance, path='auto'):
    from pyshepseg_amd import outlines
    return outlines.simplifySegmentOutlines(o, tolerance, path=path)


def by_hand(o):
    """the same rings and flags as a SegmentOutlines no trace knows: they are uploaded"""
    from pyshepseg_amd import outlines
    get = (lambda k: o[k]) if isinstance(o, dict) else (lambda k: getattr(o, k))
    return outlines.SegmentOutlines(get('maxSegId'), get('ringOffsets'), get('vertexOffsets'), get('vertices'), get('ringArea2'),
                                    junction=get('junction'))


def same(a, b):
    a = np.asarray(a)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def assert_trace(o, want):
    assert o.maxSegId == want['maxSegId']
    for k in RINGS + ('junction',):
        assert same(getattr(o, k), want[k]), k
    assert o.junction.dtype == np.uint8


def assert_simplified(got, want, uploaded=None):
    from pyshepseg_amd import outlines
    assert isinstance(got, outlines.SimplifiedOutlines)
    for k in RESULT:
        assert same(getattr(got, k), want[k]), k
    assert (got.rounds, got.arcs, got.longestArc) == (want['rounds'], want['arcs'], want['longestArc'])
    assert sum(got.arcClasses.values()) == got.arcs and sorted(got.deviceStepsMs) == sorted(outlines.SIMPLIFY_STEPS)
    assert got.deviceMs >= 0 and got.residentSerial is None
    if uploaded is not None:
        assert got.timings['uploaded'] == uploaded


@functools.lru_cache(maxsize=None)
def raster(name):
    if name == 'example':
        seg = oc.EXAMPLE
    elif name == 'border_t':
        seg = np.array([[1, 2]], dtype=np.uint32)
    elif name == 'saddle_two_labels':
        seg = np.array([[1, 2], [2, 1]], dtype=np.uint32)
    elif name == 'saddle_with_zero':
        seg = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 3, 3, 0]], dtype=np.uint32)
    elif name.startswith('checkerboard'):
        seg = oc.checkerboard(int(name[12:]))
    elif name == 'random256':
        seg = nc.random_labels((256, 256), 2999, 2)
    elif name == 'random1024':
        seg = nc.random_labels((1024, 1024), 39999, 1)
    elif name == 'staircase':
        seg = oc.staircase(70)
    elif name == 'squares':
        seg = oc.concentric_squares()
    elif name == 'scattered':
        seg = oc.scattered_parts()
    elif name == 'zeros':
        seg = np.zeros((5, 9), dtype=np.uint32)
    elif name == 'empty':
        seg = np.zeros((0, 5), dtype=np.uint32)
    elif name == 'mosaic':
        with np.load(os.path.join(GOLDEN, 'ci_scenario_1000.npz')) as z:
            seg = z['mosaic']
    else:
        with np.load(os.path.join(GOLDEN, 'tile_synth128_null.npz')) as z:
            seg = z[name]
    seg = np.ascontiguousarray(seg, dtype=np.uint32)
    seg.setflags(write=False)
    return seg


@functools.lru_cache(maxsize=None)
def model_trace(name, four):
    return sc.reference_junction_trace(raster(name), four, maxSegId=2 if name == 'empty' else None)


@functools.lru_cache(maxsize=None)
def model_simplified(name, four, tolerance):
    return sc.reference_simplify(model_trace(name, four), tolerance)


TRACED = ('example', 'border_t', 'saddle_two_labels', 'saddle_with_zero', 'checkerboard8', 'checkerboard65', 'random256', 'seg_final')
MORE = ('staircase', 'squares', 'scattered', 'zeros', 'empty')


# ---- the junction trace -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
@pytest.mark.parametrize('name', TRACED)
def test_junction_trace(name, four):
    from pyshepseg_amd import outlines
    seg = raster(name)
    before = trace(seg, fourConnected=four)
    assert before.junction is None and before.simplified is None
    o = trace(seg, fourConnected=four, junctions=True, hulls=True)
    assert_trace(o, model_trace(name, four))
    assert same(o.ringArea2, before.ringArea2) and same(o.ringOffsets, before.ringOffsets)
    for k in ('numParts', 'numHoles', 'holeArea'):
        assert same(o.columns[k], before.columns[k]), k
    assert np.all(o.columns['numVertices'] >= before.columns['numVertices']) and o.edges == before.edges
    # the junction vertices are collinear or vertices anyway: the hulls are the plain trace's, in place and uploaded
    plain_hulls = outlines.calcSegmentHulls(before)
    for h in (o.hulls, outlines.calcSegmentHulls(by_hand(o))):
        for k in ('hullOffsets', 'hullPoints', 'hullReach'):
            assert same(getattr(h, k), getattr(plain_hulls, k)), k
    assert not o.hulls.timings['uploaded']
    # the switch does not stick: a following plain trace returns the bytes it returned before
    after = trace(seg, fourConnected=four)
    assert after.junction is None
    for k in RINGS:
        assert getattr(after, k).tobytes() == getattr(before, k).tobytes(), k


def test_junction_trace_with_an_origin_and_a_given_max_id():
    o = trace(oc.EXAMPLE, junctions=True, origin=(10, 2 ** 32 - 4), maxSegId=6)
    assert_trace(o, sc.reference_junction_trace(oc.EXAMPLE, True, maxSegId=6, origin=(10, 2 ** 32 - 4)))
    s = simplify(o, 1.0)
    assert_simplified(s, sc.reference_simplify(o, 1.0), uploaded=False)
    assert s.origin == o.origin and s.maxSegId == 6 and len(s.ringOffsets) == 8


# ---- simplification against the model -----------------------------------------------------------------------------------
@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
@pytest.mark.parametrize('name', TRACED + MORE)
def test_rasters_against_the_model(name, four):
    seg = raster(name)
    o = trace(seg, fourConnected=four, junctions=True, maxSegId=2 if name == 'empty' else None)
    assert_trace(o, model_trace(name, four))
    up = by_hand(o)
    for t in sc.TOLERANCES:
        want = model_simplified(name, four, t)
        assert_simplified(simplify(o, t), want, uploaded=False)
        assert_simplified(simplify(up, t), want, uploaded=True)
    both = trace(seg, fourConnected=four, simplify=1.0, maxSegId=2 if name == 'empty' else None)
    assert both.junction is not None and 'simplify' in both.timings and both.simplified.source is both
    assert_simplified(both.simplified, model_simplified(name, four, 1.0), uploaded=False)


def test_what_the_rasters_are_there_for():
    from pyshepseg_amd import outlines
    # the staircase collapses to its diagonal
    s = trace(raster('staircase'), simplify=1.0).simplified
    assert len(s.source.vertices) > 280 and len(s.vertices) <= 9 and not s.droppedRings.any()
    assert [0, 1] in s.ring(0).tolist() and [69, 70] in s.ring(0).tolist() and [35, 35] not in s.ring(0).tolist()
    # concentric squares: closed arcs shared by a shell and a hole, which keep the same corners
    o = trace(raster('squares'), junctions=True)
    assert int(o.junction.sum()) == 0
    s = simplify(o, 1.0)
    assert same(s.vertices, o.vertices) and not s.droppedRings.any() and s.arcs == len(o.ringArea2)
    assert [len(p) for p in s.polygonsOf(1)] == [2, 2, 1] and outlines.toWKT(s, 2) == outlines.toWKT(o, 2)
    # scattered single pixels: a pixel whose four neighbours have one id has no junction, keeps only its diagonal from a
    # tolerance of sqrt(1 / 2) on and is dropped with the hole it left; a pixel between several ids keeps its four
    # junction corners
    o = trace(raster('scattered'), junctions=True)
    (one, s) = (simplify(o, 0.5), simplify(o, 1.5))
    want = model_simplified('scattered', True, 1.5)
    assert not one.droppedRings.any() and s.droppedRings.sum() == want['droppedRings'].sum() == 4
    assert same(s.columns['droppedRings'], want['droppedRings']) and s.droppedRings[7] == 0
    assert np.array_equal(s.columns['numParts'] + s.columns['numHoles'] + s.droppedRings, o.columns['numParts'] + o.columns['numHoles'])
    # no rings at all
    for name in ('zeros', 'empty'):
        s = trace(raster(name), simplify=4.0, maxSegId=2).simplified
        assert s.ringOffsets.tolist() == [0, 0, 0, 0] and s.vertices.shape == (0, 2) and s.vertexOffsets.tolist() == [0]
        assert s.rounds == 0 and s.arcs == 0


@pytest.mark.parametrize('tolerance', [1.0, 4.0])
@pytest.mark.parametrize('name', ['random1024', 'mosaic'])
def test_every_corner_has_one_kept_flag_in_all_rings(name, tolerance):
    """on random1024 (arcs of two and three points) and on the 1000 x 1000 mosaic (segments of real shapes), where the model is
    too slow to be the yardstick: among the rings that survive, a corner of the source is kept by all rings through it or by
    none"""
    o = trace(raster(name), junctions=True)
    s = simplify(o, tolerance)
    assert not s.timings['uploaded'] and 0 < len(s.vertices) < len(o.vertices)
    assert same(s.vertices, o.vertices[s.keptVertex])
    kept = np.zeros(len(o.vertices), dtype=np.int64)
    kept[s.keptVertex] = 1
    alive = np.zeros(len(o.ringArea2), dtype=bool)
    alive[s.sourceRing] = True
    inring = np.repeat(alive, np.diff(o.vertexOffsets))
    corner = (o.vertices[:, 0] * 2048 + o.vertices[:, 1])[inring]
    (_u, inv) = np.unique(corner, return_inverse=True)
    (lo, hi) = (np.ones(inv.max() + 1, dtype=np.int64), np.zeros(inv.max() + 1, dtype=np.int64))
    np.minimum.at(lo, inv, kept[inring])
    np.maximum.at(hi, inv, kept[inring])
    assert np.array_equal(lo, hi)
    assert np.all(kept[o.junction == 1][inring[o.junction == 1]] == 1)
    assert s.arcs > 500 and s.longestArc >= 3 and (s.rounds >= 1 or name != 'mosaic')


# ---- arcs built by hand -------------------------------------------------------------------------------------------------
def far_of(points):
    rows = [p[0] for p in points]
    return ((min(rows) + max(rows)) // 2, min(p[1] for p in points) - 100000)


def check_ring(ring, tolerances=(0.5, 1.5), survive=True, path='auto'):
    m = sc.outlines_from({2: [ring]}, maxSegId=3)
    out = []
    for t in tolerances:
        want = sc.reference_simplify(m, t)
        assert not survive or len(want['sourceRing']) == 1
        got = simplify(by_hand(m), t, path)
        assert_simplified(got, want, uploaded=True)
        out.append(got)
    return out


def admits(path, n):
    return path in ('auto', 'global') or n <= {'short': sc.SHORT_MAX, 'group': sc.GROUP_MAX}[path]


def class_of(path, n):
    if path == 'global':
        return 'global'
    if path == 'group':
        return 'group' if n <= sc.GROUP_MAX else 'global'
    return 'short' if n <= sc.SHORT_MAX else ('group' if n <= sc.GROUP_MAX else 'global')


@pytest.mark.parametrize('n,path', [(n, path) for n in (2, 3, 63, 64, 65, 255, 256, 257, sc.GROUP_MAX - 1, sc.GROUP_MAX, sc.GROUP_MAX + 1)
                                    for path in PATHS if admits(path, n)])
def test_arc_sizes(n, path):
    pts = sc.wobble(n)
    for got in check_ring(sc.arc_ring(pts, far=far_of(pts)), path=path):
        # the ring's other two arcs have two points
        small = class_of(path, 2)
        classes = {'short': 0, 'group': 0, 'global': 0}
        classes[small] += 2
        classes[class_of(path, n)] += 1
        assert got.arcClasses == classes and got.longestArc == max(n, 2) and got.arcs == 3


@pytest.mark.parametrize('narcs', [63, 64, 65, 2047, 2048, 2049])
def test_arc_counts(narcs):
    ring = sc.many_arcs(narcs)
    (half, one) = check_ring(ring, (0.5, 1.0))
    assert half.arcs == one.arcs == narcs and half.arcClasses['short'] == narcs
    # the points between the anchors are 1, 2 or 3 rows off their chords of length 2
    assert len(half.vertices) == len(ring[0]) and len(one.vertices) == len(ring[0]) - len(range(0, narcs - 1, 3))


@pytest.mark.parametrize('path', PATHS)
def test_wrapping_arcs_single_anchors_and_rings_of_anchors(path):
    pts = sc.wobble(40)
    for wrap in (1, 7, 39, 40):
        check_ring(sc.arc_ring(pts, wrap=wrap, far=far_of(pts)), path=path)
    # no flag at all: one closed arc from the vertex of the smallest (row, col), which is not the first of the list
    (verts, flags) = sc.arc_ring(pts, wrap=9, far=far_of(pts))
    for got in check_ring((verts, [0] * len(verts)), path=path):
        assert got.arcs == 1 and got.longestArc == len(verts) + 1
        assert list(min(verts)) in got.ring(0).tolist()
    # every vertex an anchor: nothing can go
    for got in check_ring((verts, [1] * len(verts)), (0.0, 4.0), path=path):
        assert got.arcs == len(verts) and same(got.keptVertex, np.arange(len(verts), dtype=np.int64)) and got.rounds == 0
    # several rings of several ids at once, one of them without vertices to keep
    m = sc.outlines_from({1: [sc.arc_ring(sc.wobble(70), far=far_of(sc.wobble(70))), ([(0, 0), (0, 1), (1, 1), (1, 0)], [0, 0, 0, 0])],
                          4: [sc.arc_ring(sc.wobble(5, 1), wrap=2, far=far_of(sc.wobble(5, 1))), ([(5, 5), (5, 6), (6, 6)], [1, 0, 0])]},
                         maxSegId=5)
    for t in sc.TOLERANCES:
        assert_simplified(simplify(by_hand(m), t, path), sc.reference_simplify(m, t), uploaded=True)
    assert simplify(by_hand(m), 4.0, path).droppedRings.tolist() == [0, 1, 0, 0, 1, 0]


@pytest.mark.parametrize('path', ['group', 'global'])
@pytest.mark.parametrize('n', [65, 300])
def test_depth(n, path):
    pts = sc.zigzag(n)
    (got,) = check_ring(sc.arc_ring(pts, far=far_of(pts)), (0.5,), path=path)
    assert got.rounds == n - 2 == sc.simplify_arc(pts, sc.tolerance2q(0.5))[1]
    assert len(got.vertices) == n + 1


# ---- ties and limits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', PATHS)
def test_ties_and_the_boundary_of_the_tolerance(path):
    from pyshepseg_amd import outlines
    for arc in (sc.TIE_ARC, sc.TIE_ARC[::-1]):
        (got,) = check_ring(sc.arc_ring(arc, far=far_of(arc)), (1.0,), path=path)
        assert len(got.vertices) == 6 and got.rounds == 3
    # (1, 1) over the chord (0, 0) - (0, 2): m^2 65536 = 4 * 65536 = T |b - a|^2 at T = 65536, where it is not kept
    arc = [(0, 0), (1, 1), (0, 2)]
    below = math.sqrt(65535.5 / 65536.0)
    assert outlines.tolerance2q(1.0) == 65536 and outlines.tolerance2q(below) == 65535
    (on, under) = check_ring(sc.arc_ring(arc, far=(50, -1000)), (1.0, below), path=path)
    assert (on.tolerance2q, under.tolerance2q) == (65536, 65535)
    assert len(on.vertices) == 3 and len(under.vertices) == 4 and [1, 1] in under.vertices.tolist()
    # the same on a closed arc: |q - a|^2 65536 > T, with |q - a|^2 = 16 for both other corners
    tri = ([(0, 0), (0, 4), (4, 0)], [0, 0, 0])
    below = math.sqrt((16 * 65536 - 0.5) / 65536.0)
    assert outlines.tolerance2q(4.0) == 16 * 65536 and outlines.tolerance2q(below) == 16 * 65536 - 1
    (on, under) = check_ring(tri, (4.0, below), survive=False, path=path)
    assert len(on.vertices) == 0 and on.droppedRings.tolist() == [0, 0, 1, 0]
    assert under.ring(0).tolist() == [[0, 0], [0, 4], [4, 0]] and under.rounds == 2


def test_coordinates_at_the_span_limits():
    """H = 2^31 - 1 and W = 2: cross products of 2^32, whose squares times 65536 take 81 bits, against chords of squared
    length 2^62; the distances from the chord lie within a few 2^-31 of 1 and 2"""
    top = 2 ** 31 - 1
    arc = [(0, 0), (2 ** 27, 1), (2 ** 28, 2), (2 ** 29, 1), (2 ** 30, 2), (2 ** 30 + 5, 1), (top - 2 ** 20, 2), (top - 1, 2), (top, 1)]
    ring = sc.arc_ring(arc, far=(2 ** 30, 0))
    tolerances = (0.5, 0.9999999, 1.0, 1.0000001, 1.5, 1.9999999, 2.0, 32768.0)
    got = check_ring(ring, tolerances)
    assert len({len(g.vertices) for g in got}) >= 3
    moved = ([(r - 2 ** 40, c + 2 ** 50) for (r, c) in ring[0]], ring[1])
    for (g, h) in zip(got, check_ring(moved, tolerances)):
        assert same(g.keptVertex, h.keptVertex)
    # a closed arc across the whole span: squared distances of 2^62
    sq = ([(0, 0), (0, 2), (top, 2), (top, 0)], [0, 0, 0, 0])
    (whole, none) = check_ring(sq, (0.0, 32768.0), survive=False)
    assert len(whole.vertices) == 4 and len(none.vertices) == 0


# ---- entry points -----------------------------------------------------------------------------------------------------
def test_call_order_is_enforced_and_the_other_state_stays():
    from pyshepseg_amd import _lib, neighbours, outlines
    nb = neighbours.findSegmentNeighbours(nc.EXAMPLE, True)
    serial = neighbours.residentTableSerial()
    c = _lib.ctx()
    L = c._L
    counts = np.full(10, 7, dtype=np.int64)
    out = [np.full(64, 7, dtype=np.int64) for _k in range(6)]

    def refused(rc, what):
        assert rc != 0
        assert what in L.shp_last_error(c.handle).decode()

    def source_call():
        return L.shp_simplify_source(c.handle, None, None, None, None, None, 0, 0, 0, None)

    def build_call(T=65536, path=0):
        return L.shp_simplify_build(c.handle, T, path, 0, 0, 3, 3, _lib.ptr(counts), None)

    def download_call():
        return L.shp_simplify_download(c.handle, *[_lib.ptr(a) for a in out])
    (edges, bad) = (ctypes.c_int64(0), ctypes.c_uint32(0))
    trace(oc.EXAMPLE)
    refused(L.shp_outline_junctions(c.handle, 1), 'shp_outline_edges_dev must come first')
    c.check(L.shp_outline_edges_dev(c.handle, None, 0, 0, 0, 1, ctypes.byref(edges), ctypes.byref(bad)))
    refused(source_call(), 'shp_outline_trace must come first')
    refused(build_call(), 'shp_simplify_source must come first')
    refused(download_call(), 'shp_simplify_build must come first')
    flags = np.full(64, 7, dtype=np.uint8)
    refused(L.shp_outline_download_junction(c.handle, _lib.ptr(flags)), 'shp_outline_trace must come first')
    assert counts.tolist() == [7] * 10 and out[0][0] == 7 and flags[0] == 7
    plain = trace(oc.EXAMPLE)
    refused(source_call(), 'shp_outline_junctions must come first')
    refused(L.shp_outline_download_junction(c.handle, _lib.ptr(flags)), 'shp_outline_junctions must come first')
    assert plain.junction is None
    o = trace(oc.EXAMPLE, junctions=True, hulls=True)
    c.check(L.shp_outline_download_junction(c.handle, _lib.ptr(flags)))
    assert flags[:19].tolist() == o.junction.tolist() and flags[19] == 7
    c.check(source_call())
    refused(download_call(), 'shp_simplify_build must come first')
    refused(L.shp_simplify_build(c.handle, 65536, 0, 0, 0, 3, 3, None, None), 'NULL')
    refused(build_call(T=2 ** 46 + 1), 'tolerance2q')
    refused(build_call(path=4), 'path')
    refused(L.shp_simplify_build(c.handle, 65536, 0, 0, 0, 2 ** 31, 1, _lib.ptr(counts), None), 'spans')
    c.check(build_call())
    want = sc.reference_simplify(o, 1.0)
    assert counts[:5].tolist() == [3, 10, want['rounds'], want['arcs'], want['longestArc']]
    assert counts[5:].tolist() == [want['arcs'], 0, 0, 10, 0]
    refused(L.shp_simplify_download(c.handle, None, None, None, None, None, None), 'NULL')
    c.check(download_call())
    assert out[0][:5].tolist() == want['ringOffsets'].tolist() and out[1][:4].tolist() == want['vertexOffsets'].tolist()
    assert out[2][:20].reshape(10, 2).tolist() == want['vertices'].tolist() and out[3][:3].tolist() == want['ringArea2'].tolist()
    assert out[4][:3].tolist() == [0, 1, 2] and out[5][:10].tolist() == want['keptVertex'].tolist() and out[5][10] == 7
    # the outlines, the hulls and the neighbour table are still there and the same
    rings = [np.full(64, 7, dtype=np.int64) for _k in range(4)]
    c.check(L.shp_outline_download(c.handle, *[_lib.ptr(a) for a in rings]))
    assert rings[0][:5].tolist() == [0, 0, 1, 2, 3] and rings[3][:3].tolist() == oc.EXAMPLE_AREA2
    assert np.array_equal(rings[2][:38].reshape(19, 2), o.vertices)
    hull = [np.full(64, 7, dtype=np.int64) for _k in range(5)]
    c.check(L.shp_hull_download(c.handle, *[_lib.ptr(a) for a in hull]))
    assert np.array_equal(hull[0][:5], o.hulls.hullOffsets) and np.array_equal(hull[1][:30].reshape(15, 2), o.hulls.hullPoints)
    assert neighbours.residentTableSerial() == serial
    red = neighbours.reduceOverNeighbours(nb, [(np.arange(4, dtype=np.float64), [('n', 'count')])])
    assert red['n'].tolist() == [0, 2, 2, 2] and not nb.reduceTimings['uploaded']
    assert not outlines.calcSegmentHulls(o).timings['uploaded'] and not simplify(o, 0.5).timings['uploaded']
    # a resident source whose outlines are replaced before the build
    c.check(source_call())
    c.check(L.shp_outline_edges_dev(c.handle, None, 0, 0, 0, 1, ctypes.byref(edges), ctypes.byref(bad)))
    refused(build_call(), 'the traced outlines have been replaced')
    refused(build_call(), 'shp_simplify_source must come first')
    # uploaded arrays that do not fit
    (ro, vo) = (o.ringOffsets, o.vertexOffsets.copy())
    args = lambda ro_, vo_, S=3: (c.handle, _lib.ptr(ro_), _lib.ptr(vo_), _lib.ptr(o.vertices), _lib.ptr(o.ringArea2),  # noqa: E731
                                  _lib.ptr(o.junction), S, 3, 19, None)
    vo[-1] = 18
    refused(L.shp_simplify_source(*args(ro, vo)), 'do not span')
    vo[-1] = 19
    vo[1] = 15
    refused(L.shp_simplify_source(*args(ro, vo)), 'do not ascend')
    refused(L.shp_simplify_source(c.handle, _lib.ptr(ro), _lib.ptr(o.vertexOffsets), _lib.ptr(o.vertices), _lib.ptr(o.ringArea2), None,
                                  3, 3, 19, None), 'NULL')
    refused(L.shp_simplify_source(*args(ro, o.vertexOffsets, S=-1)), 'max_seg_id')
    # o's rings are no longer resident: the function sees that and uploads
    got = simplify(o, 1.0)
    assert_simplified(got, want, uploaded=True)


def test_working_set_is_refused_before_it_is_allocated(monkeypatch):
    from pyshepseg_amd import _lib, outlines
    c = _lib.ctx()
    o = trace(oc.EXAMPLE, junctions=True)

    class Library(object):
        """the library, whose simplification buffers would have to grow by a terabyte more"""
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            fn = getattr(c._L, name)

            def call(*args):
                self.calls.append(name)
                rc = fn(*args)
                if name == 'shp_simplify_need':
                    args[5]._obj.value += 10 ** 12
                return rc
            return call

    class Ctx(object):
        def __init__(self):
            (self.handle, self.check, self._L) = (c.handle, c.check, Library())
    fake = Ctx()
    monkeypatch.setattr(_lib, 'ctx', lambda: fake)
    with pytest.raises(outlines.PyShepSegOutlinesError,
                       match=r'the simplification arrays of 19 vertices, 3 rings and 4 ids need 1\d{12} bytes of device memory, \d+ are free'):
        outlines.simplifySegmentOutlines(o, 1.0)
    assert fake._L.calls == ['shp_outline_serial', 'shp_simplify_need']
    monkeypatch.undo()
    assert not simplify(o, 1.0).timings['uploaded']     # nothing was launched or replaced: o is still resident
    # the bytes follow the counts as stated
    (need, free) = (ctypes.c_int64(0), ctypes.c_int64(0))
    big = 2 ** 26
    c.check(c._L.shp_simplify_need(c.handle, big, big // 4, 1000, 0, ctypes.byref(need), ctypes.byref(free)))
    assert 100 * big <= need.value <= 180 * big * 9 // 8 + 2 ** 24
    c.check(c._L.shp_simplify_need(c.handle, big, big // 4, 1000, 1, ctypes.byref(need), ctypes.byref(free)))
    assert (100 + 17 + 4) * big <= need.value <= (180 + 17 + 4) * big * 9 // 8 + 2 ** 24
    assert c._L.shp_simplify_need(c.handle, 2 ** 31, 1, 1, 0, ctypes.byref(need), ctypes.byref(free)) != 0


def test_the_calls_of_a_trace(monkeypatch):
    from pyshepseg_amd import _lib, outlines
    c = _lib.ctx()

    class Recorder(object):
        def __init__(self):
            (self.handle, self.check, self._L, self.calls) = (c.handle, c.check, self, [])

        def __getattr__(self, name):
            self.calls.append(name)
            return getattr(c._L, name)
    fake = Recorder()
    monkeypatch.setattr(_lib, 'ctx', lambda: fake)
    plain = ['shp_outline_need', 'shp_outline_edges_dev', 'shp_outline_need', 'shp_outline_trace', 'shp_outline_download']
    outlines.traceSegmentOutlines(oc.EXAMPLE, maxSegId=3)
    assert [n for n in fake.calls if n.startswith(('shp_outline', 'shp_hull', 'shp_simplify'))] == plain
    fake.calls = []
    outlines.traceSegmentOutlines(oc.EXAMPLE, maxSegId=3, junctions=True)
    assert [n for n in fake.calls if n.startswith(('shp_outline', 'shp_hull', 'shp_simplify'))] == \
        plain[:2] + ['shp_outline_junctions'] + plain[2:] + ['shp_outline_download_junction']
    fake.calls = []
    outlines.traceSegmentOutlines(oc.EXAMPLE, maxSegId=3, simplify=1.0)
    assert [n for n in fake.calls if n.startswith('shp_simplify')] == ['shp_simplify_need', 'shp_simplify_source', 'shp_simplify_build',
                                                                       'shp_simplify_download']


def test_readme_example(tmp_path):
    """the README's lines: the junction trace simplified, its columns, hulls and export, and both in one call"""
    from pyshepseg_amd import outlines
    with np.load(os.path.join(GOLDEN, 'ci_scenario_1000.npz')) as z:
        seg = np.ascontiguousarray(z['mosaic'], dtype=np.uint32)
    o = outlines.traceSegmentOutlines(seg, junctions=True)
    s = outlines.simplifySegmentOutlines(o, 1.5)
    cols = dict(s.columns)
    cols.update(outlines.calcSegmentHulls(s).columns)
    wkt = outlines.toWKT(s, 42)
    n = outlines.writeGeoJSON(s, str(tmp_path / 'simplified.geojson'), ids=[42, 43], columns={'droppedRings': s.droppedRings})
    assert n == 2 and wkt.startswith('MULTIPOLYGON') and len(s.vertices) < len(o.vertices)
    assert cols['numVertices'][42] == sum(len(r) for r in s.ringsOf(42)) and len(cols['solidity']) == o.maxSegId + 1
    assert same(s.vertices, o.vertices[s.keptVertex]) and s.tolerance == 1.5 and s.tolerance2q == 147456
    both = outlines.traceSegmentOutlines(seg, simplify=1.5).simplified
    for k in RESULT:
        assert same(getattr(both, k), getattr(s, k)), k
