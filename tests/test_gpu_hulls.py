"""GPU: outlines.calcSegmentHulls against the sequential model (tests/hull_cases.py): numpy.array_equal on every integer
array, dtype included; the float columns, which the host derives from those integers, at rtol 1e-12 against the model's
math.fsum values (the hulls here have at most a few thousand edges, and a float64 sum of h terms errs by about h 2^-53).

The kernels (csrc/hull.h) take a vertex, a candidate, an id or a hull edge per thread in workgroups of 256, the chains a
wavefront per id; the shared scan takes 8192 items a workgroup and the shared sort 2048.  The one size threshold is
HL_WAVE_MAX = 64 kept points of an id: up to it the chains are built in registers, beyond it by one lane's stack.  A
histogram ring of n + 2 columns keeps 2 (n + 3) points, so test_pop_cascade's n = 28, 29, 30 lie at 62, 64 and 66 kept
points; its variants with two level tops and a triangle keep 2 n + 5: 63 and 65 at n = 29 and 30.

Rings a trace made are hulled twice, read in place (only convex corners of outer rings are candidates) and uploaded
(every vertex is one): both must give the model's arrays."""
import ctypes
import functools
import os

import numpy as np
import pytest

import hull_cases as hc
import neighbour_cases as nc
import outline_cases as oc
import simplify_cases as sc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ARRAYS = ('hullOffsets', 'hullPoints', 'hullReach')
RTOL = 1e-12


def trace(seg, **kw):
    from pyshepseg_amd import outlines
    return outlines.traceSegmentOutlines(seg, **kw)


def hulls(o, **kw):
    from pyshepseg_amd import outlines
    return outlines.calcSegmentHulls(o, **kw)


def by_hand(o):
    """the same rings as a SegmentOutlines no trace knows: they are uploaded"""
    from pyshepseg_amd import outlines
    return outlines.SegmentOutlines(o.maxSegId, o.ringOffsets, o.vertexOffsets, o.vertices, o.ringArea2, origin=o.origin,
                                    fourConnected=o.fourConnected)


def assert_equal(got, want):
    """two SegmentHulls: every array and column, bit for bit"""
    assert got.maxSegId == want.maxSegId
    for k in ARRAYS:
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    assert sorted(got.columns) == sorted(want.columns)
    for k in got.columns:
        assert got.columns[k].dtype == want.columns[k].dtype and np.array_equal(got.columns[k], want.columns[k]), k


def assert_same(got, want):
    """want: the model's dictionary"""
    assert got.maxSegId == want['maxSegId']
    for k in ARRAYS:
        a = getattr(got, k)
        assert a.dtype == np.int64 and a.shape == want[k].shape and np.array_equal(a, want[k]), k
    assert sorted(got.sums) == sorted(hc.SUMS) and sorted(got.columns) == sorted(hc.SUMS + hc.DERIVED)
    for k in hc.SUMS:
        assert got.sums[k].dtype == np.int64 and np.array_equal(got.sums[k], want['sums'][k]), k
        assert got.columns[k] is got.sums[k]
    for k in hc.DERIVED:
        assert got.columns[k].dtype == np.float64
        assert np.allclose(got.columns[k], want['columns'][k], rtol=RTOL, atol=0.0), k
    assert got.deviceMs >= 0 and sorted(got.deviceStepsMs) == sorted(('candidates', 'order', 'chains', 'points', 'reach'))


def check_rings(o):
    got = hulls(o)
    assert got.timings['uploaded']
    assert_same(got, hc.reference_hulls(o))
    return got


def check_raster(seg, fourConnected=True, maxSegId=None, origin=(0, 0)):
    """traced, hulled in place and once more uploaded; both against the model"""
    o = trace(seg, fourConnected=fourConnected, maxSegId=maxSegId, origin=origin)
    want = hc.reference_hulls(o)
    got = hulls(o)
    assert not got.timings['uploaded']
    assert_same(got, want)
    up = hulls(by_hand(o))
    assert up.timings['uploaded']
    assert_same(up, want)
    assert got.candidates <= up.candidates == len(o.vertices) and got.kept <= got.candidates
    return got


@functools.lru_cache(maxsize=None)
def real_raster(name):
    if name == 'mosaic':
        with np.load(os.path.join(GOLDEN, 'ci_scenario_1000.npz')) as z:
            seg = z['mosaic']
    elif name == 'random1024':
        seg = nc.random_labels((1024, 1024), 39999, 1)
    elif name == 'random256':
        seg = nc.random_labels((256, 256), 2999, 2)
    else:
        with np.load(os.path.join(GOLDEN, 'tile_synth128_null.npz')) as z:
            seg = z[name]
    seg = np.ascontiguousarray(seg, dtype=np.uint32)
    seg.setflags(write=False)
    return seg


# ---- worked examples --------------------------------------------------------------------------------------------------
def test_worked_examples():
    got = check_raster(oc.EXAMPLE)
    assert got.hullOf(1).tolist() == [[0, 0], [0, 2], [1, 2], [2, 1], [2, 0]] and got.sums['hullArea2'].tolist() == [0, 7, 10, 4]
    assert got.hullOf(3).tolist() == [[2, 0], [2, 2], [3, 2], [3, 0]] and got.hullOf(0).shape == (0, 2)
    assert got.deviceMs > 0 and got.timings['total'] > 0
    got = check_raster(np.ones((1, 1), dtype=np.uint32))
    assert (got.sums['hullArea2'][1], got.sums['feretMax2'][1], got.columns['feretMin'][1], got.columns['solidity'][1]) == (2, 2, 1.0, 1.0)
    for shape in ((1, 37), (37, 1), (5, 9)):
        got = check_raster(np.ones(shape, dtype=np.uint32))
        assert got.columns['solidity'][1] == 1.0 and got.columns['feretMin'][1] == float(min(shape))
        assert got.sums['feretMax2'][1] == shape[0] ** 2 + shape[1] ** 2 and got.hullReach.tolist() == [shape[0] * shape[1]] * 4
    got = check_raster(hc.L_SHAPE)
    assert got.hullOf(1).tolist() == [[0, 0], [0, 1], [2, 3], [3, 3], [3, 0]] and got.columns['solidity'][1] == 5.0 / 7.0
    got = check_raster(hc.PLUS)
    assert got.sums['numHullVertices'][1] == 8 and got.hullReach.tolist() == [3, 4] * 4
    # a hole changes the solidity and not the hull
    ring = check_raster(hc.RING)
    full = check_raster(np.where(hc.RING == 0, 1, hc.RING).astype(np.uint32))
    assert np.array_equal(ring.hullOf(1), full.hullOf(1)) and ring.sums['hullArea2'][1] == 32
    assert ring.columns['solidity'][1] == 12.0 / 16.0 and full.columns['solidity'][1] == 15.0 / 16.0


# ---- collinear and repeated points ------------------------------------------------------------------------------------
def test_collinear_and_repeated_points():
    got = check_raster(oc.staircase())
    assert got.hullOf(1).tolist() == [[0, 0], [0, 1], [69, 70], [70, 70], [70, 0]]      # every step's corner on the diagonal edge
    got = check_raster(hc.diamond(40))
    assert got.sums['numHullVertices'][1] == 8
    # two pixels of one id that touch diagonally: with four-connected rings the corner belongs to both rings
    seg = np.array([[1, 0], [0, 1]], dtype=np.uint32)
    o = trace(seg)
    assert len(o.ringArea2) == 2 and [1, 1] in o.ring(0).tolist() and [1, 1] in o.ring(1).tolist()
    got = check_raster(seg)
    assert got.hullOf(1).tolist() == [[0, 0], [0, 1], [1, 2], [2, 2], [2, 1], [1, 0]]
    # the same ring twice, and a ring with a vertex repeated and collinear vertices left in
    sq = hc.rectangle_ring(3, 4, 2, 5)
    got = check_rings(hc.outlines_from_rings({1: [sq, sq], 4: [[(0, 0), (0, 2), (0, 2), (0, 5), (3, 5), (3, 5), (3, 0), (1, 0)]]}))
    assert got.hullOf(1).tolist() == [list(p) for p in sq] and got.sums['numHullVertices'].tolist() == [0, 4, 0, 0, 4]


# ---- several parts, both corner rules ---------------------------------------------------------------------------------
def test_several_parts_form_one_hull():
    got = check_raster(oc.scattered_parts())
    assert 4 < got.sums['numHullVertices'][7] < 40
    for four in (True, False):
        got = check_raster(oc.checkerboard(8), four)
        # the whole square but for the two corner pixels of label 0, whichever way the diagonal contacts are cut
        assert got.hullOf(1).tolist() == [[0, 1], [0, 8], [7, 8], [8, 7], [8, 0], [1, 0]]


@pytest.mark.parametrize('name', ['mosaic', 'seg_final', 'random1024', 'random256'])
def test_the_corner_rule_does_not_change_the_hulls(name):
    seg = real_raster(name)
    (a, b) = (trace(seg, fourConnected=True, hulls=True).hulls, trace(seg, fourConnected=False, hulls=True).hulls)
    for k in ARRAYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for k in hc.SUMS:
        assert np.array_equal(a.sums[k], b.sums[k]), k


# ---- bounded by the vertices ------------------------------------------------------------------------------------------
def test_work_and_memory_follow_the_vertices_not_the_bounding_box():
    from pyshepseg_amd import _lib
    seg = hc.end_pixels(64, 4097)
    got = check_raster(seg)
    assert got.sums['numHullVertices'][1:].tolist() == [4] * 64 and got.sums['hullArea2'][1:].tolist() == [2 * 4097] * 64
    c = _lib.ctx()
    (need, free) = (ctypes.c_int64(0), ctypes.c_int64(0))
    (nverts, nrings, S) = (64 * 8, 128, 64)
    for upload in (0, 1):
        c.check(c._L.shp_hull_need(c.handle, nverts, nrings, S, upload, ctypes.byref(need), ctypes.byref(free)))
        # at most 96 bytes a vertex, 16 a ring, 48 an id and the buffers' fixed parts: less than a byte a pixel of the
        # 64 x 4097 bounding boxes
        assert 0 <= need.value <= 200 * nverts + 64 * (nrings + S) + 2 ** 16 < seg.size
    # the bytes grow with the counts as stated, whatever the buffers already hold
    big = 2 ** 28
    c.check(c._L.shp_hull_need(c.handle, big, big // 4, 1000, 0, ctypes.byref(need), ctypes.byref(free)))
    # 64 bytes a vertex and the sort's histograms (a byte a vertex), each buffer with the eighth the buffers grow by;
    # from below only the 48 bytes of the hulls' own buffers count, which nothing else grows (the sort's 16 and the
    # scratch may be there already from other calls of the process), less what this file's rasters left: under 2^28
    assert 47 * big <= need.value <= 66 * big * 9 // 8 + 2 ** 24
    c.check(c._L.shp_hull_need(c.handle, big, big // 4, 1000, 1, ctypes.byref(need), ctypes.byref(free)))
    assert (47 + 16 + 4) * big <= need.value <= (66 + 16 + 4) * big * 9 // 8 + 2 ** 24
    assert c._L.shp_hull_need(c.handle, 2 ** 32, 1, 1, 0, ctypes.byref(need), ctypes.byref(free)) != 0


# ---- the pop cascade, on both sides of HL_WAVE_MAX --------------------------------------------------------------------
@pytest.mark.parametrize('n', [2, 3, 28, 29, 30, 62, 63, 64, 65, 255, 256, 257])
def test_pop_cascade(n):
    rings = {}
    i = 1
    for flat in (False, True):
        ring = hc.histogram_ring(hc.cascade_heights(n, flat))
        extent = tuple(np.array(ring).max(axis=0).tolist())
        # (the level variant has no vertex in column 1: a triangle inside the body puts a single point there, which
        # makes the number of kept points odd)
        more = [[(extent[0] - 1, 1), (extent[0], 0), (extent[0], 2)]] if flat else []
        for (rows, cols) in ((False, False), (True, False), (False, True), (True, True)):
            rings[i] = [hc.mirrored(r, rows, cols, extent) for r in [ring] + more]
            i += 2
    got = check_rings(hc.outlines_from_rings(rings))
    # the tops before the last column are all popped: first top, last column (two points), the base (two points)
    assert got.sums['numHullVertices'][1] == 5 and got.kept == 8 * 2 * (n + 3) - 4
    top = 3 * n * n + 11
    assert got.hullOf(1).tolist() == [[0, n + 1], [0, n + 2], [top, n + 2], [top, 0], [top - 1, 0]]


def test_one_long_cascade():
    """1024 strictly convex tops popped by the last column, on one lane's stack"""
    ring = hc.histogram_ring(hc.cascade_heights(1024))
    got = check_rings(hc.outlines_from_rings({3: [hc.mirrored(ring, True, True)]}, maxSegId=5))
    assert got.sums['numHullVertices'].tolist() == [0, 0, 0, 5, 0, 0] and got.kept == 2 * 1027


# ---- counts round the shared blocks -----------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [63, 64, 65, 255, 256, 257, 2047, 2048, 2049])
def test_one_pixel_ids(n):
    """n hulls of four points: 4 n candidates (8192 at n = 2048, the scan block), n ids"""
    for seg in (np.arange(1, n + 1, dtype=np.uint32).reshape(1, n), np.arange(1, n + 1, dtype=np.uint32).reshape(n, 1),
                np.arange(n, 0, -1, dtype=np.uint32).reshape(1, n)):
        got = check_raster(seg)
        assert got.candidates == 4 * n and len(got.hullPoints) == 4 * n and got.sums['feretMax2'][1:].tolist() == [2] * n


# ---- reach and diameter -----------------------------------------------------------------------------------------------
def test_reach_and_diameter():
    got = check_raster(hc.parallelogram(200, 3))
    assert got.hullOf(1).tolist() == [[0, 0], [0, 3], [199, 202], [200, 202], [200, 199], [1, 0]]
    assert got.sums['feretMax2'][1] == 200 ** 2 + 202 ** 2 and got.columns['feretMin'][1] == pytest.approx(np.sqrt(8), rel=RTOL)
    got = check_raster(np.ones((30, 70), dtype=np.uint32))             # every edge has a parallel opposite edge
    assert got.hullReach.tolist() == [2100] * 4 and got.sums['feretMax2'][1] == 30 ** 2 + 70 ** 2
    # a disc: over a hundred hull edges of many directions (the diamond above has eight)
    (y, x) = np.indices((401, 401)) - 200
    got = check_raster((y * y + x * x <= 200 * 200).astype(np.uint32))
    assert got.sums['numHullVertices'][1] >= 100 and 400 ** 2 < got.sums['feretMax2'][1] < 403 ** 2


# ---- coordinates ------------------------------------------------------------------------------------------------------
def test_origin_moves_the_points_and_nothing_else():
    far = 2 ** 32 - 3               # the largest origin a raster of three rows and columns can have
    for (seg, shift) in ((oc.scattered_parts(), [10, 1000]), (oc.EXAMPLE, [far, far]), (oc.EXAMPLE, [0, far])):
        here = check_raster(seg)
        h = check_raster(seg, origin=tuple(shift))
        assert np.array_equal(h.hullPoints, here.hullPoints + np.array(shift, dtype=np.int64)) and h.hullPoints.max() >= shift[1]
        assert np.array_equal(h.hullOffsets, here.hullOffsets) and np.array_equal(h.hullReach, here.hullReach)
        for k in here.columns:
            assert np.array_equal(h.columns[k], here.columns[k]), k


def test_coordinate_limits(monkeypatch):
    from pyshepseg_amd import _lib, outlines
    got = check_rings(hc.outlines_from_rings({1: [hc.rectangle_ring(5, 5, 2 ** 31 - 1, 2)], 2: [hc.rectangle_ring(9, 6, 3, 1)]}))
    assert got.sums['hullArea2'].tolist() == [0, 4 * (2 ** 31 - 1), 6] and got.sums['feretMax2'][1] == (2 ** 31 - 1) ** 2 + 4
    got = check_rings(hc.outlines_from_rings({1: [hc.rectangle_ring(0, -7, 2 ** 16, 2 ** 16)]}, origin=(-2 ** 40, 3)))
    assert got.hullReach.tolist() == [2 ** 32] * 4
    c = _lib.ctx()

    class Recorder(object):
        def __init__(self):
            (self.handle, self.check, self._L, self.calls) = (c.handle, c.check, self, [])

        def __getattr__(self, name):
            self.calls.append(name)
            return getattr(c._L, name)
    fake = Recorder()
    monkeypatch.setattr(_lib, 'ctx', lambda: fake)
    with pytest.raises(outlines.PyShepSegOutlinesError, match='span 65536 rows and 65537 columns'):
        hulls(hc.outlines_from_rings({1: [hc.rectangle_ring(0, 0, 2 ** 16, 2 ** 16 + 1)]}))
    assert fake.calls == []


# ---- ids --------------------------------------------------------------------------------------------------------------
def test_label_zero_only_empty_rasters_sparse_and_wide_ids():
    got = check_raster(np.zeros((5, 9), dtype=np.uint32))
    assert got.hullOffsets.tolist() == [0, 0] and got.hullPoints.shape == (0, 2) and got.sums['feretMax2'].tolist() == [0]
    for shape in ((0, 5), (5, 0)):
        got = check_raster(np.zeros(shape, dtype=np.uint32), maxSegId=2)
        assert got.hullOffsets.tolist() == [0, 0, 0, 0] and got.columns['solidity'].tolist() == [-9999.0] * 3
    got = check_raster(oc.sparse_ids(), maxSegId=oc.SPARSE_MAX)
    assert np.count_nonzero(got.sums['numHullVertices']) == 3 and len(got.hullOffsets) == oc.SPARSE_MAX + 2
    check_raster(oc.wide_ids(), False, maxSegId=oc.WIDE_MAX)
    o = trace(oc.EXAMPLE, maxSegId=5)
    assert hulls(o, missing=-1.0).columns['feretMin'].tolist() == [-1.0, 2.0, 2.0, 1.0, -1.0, -1.0]


# ---- identities on real label rasters ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['mosaic', 'seg_final', 'random1024'])
def test_identities(name):
    from pyshepseg_amd import shapes
    seg = real_raster(name)
    o = trace(seg)
    h = hulls(o)
    assert not h.timings['uploaded']
    s = shapes.calcSegmentShapes(seg)
    (ro, vo, ho) = (o.ringOffsets, o.vertexOffsets, h.hullOffsets)
    area = s.columns['area']
    outer = np.concatenate([[0], np.cumsum(np.where(o.ringArea2 > 0, o.ringArea2, 0))])
    assert np.all(h.sums['hullArea2'] >= outer[ro[1:]] - outer[ro[:-1]])
    assert np.array_equal(h.sums['numHullVertices'] > 0, area > 0) and np.all(h.sums['numHullVertices'][area > 0] >= 4)
    has = area > 0
    assert np.all(h.columns['feretMin'][has] <= h.columns['feretMax'][has]) and np.all(h.columns['feretMin'][has] >= 1.0)
    assert np.all((h.columns['solidity'][has] > 0) & (h.columns['solidity'][has] <= 1))
    assert np.all(h.columns['convexity'][has] > 0)      # (above 1 where an id's parts lie apart)
    assert np.all(h.columns['solidity'][~has] == -9999.0)
    height = s.columns['rowMax'] - s.columns['rowMin'] + 1
    width = s.columns['colMax'] - s.columns['colMin'] + 1
    assert np.all(h.sums['feretMax2'][has] >= (height[has] ** 2 + 0)) and np.all(h.sums['feretMax2'][has] >= width[has] ** 2)
    assert np.all(h.sums['feretMax2'][has] <= height[has] ** 2 + width[has] ** 2)
    # every ring vertex on or inside its id's hull, every hull strictly convex and positively oriented
    for i in np.flatnonzero(has).tolist():
        p = h.hullPoints[ho[i]:ho[i + 1]]
        q = np.roll(p, -1, axis=0)
        v = o.vertices[vo[ro[i]]:vo[ro[i + 1]]]
        e = q - p
        side = e[:, 1][:, None] * (v[:, 0][None, :] - p[:, 0][:, None]) - e[:, 0][:, None] * (v[:, 1][None, :] - p[:, 1][:, None])
        assert side.min() >= 0, i
        assert np.array_equal(side.max(axis=1), h.hullReach[ho[i]:ho[i + 1]]), i
        n = np.roll(q, -1, axis=0) - q
        assert np.all(e[:, 1] * n[:, 0] - e[:, 0] * n[:, 1] > 0), i
    # hulling the hulls returns them
    from pyshepseg_amd import outlines
    again = hulls(outlines.SegmentOutlines(o.maxSegId, np.concatenate([[0], np.cumsum(has.astype(np.int64))]),
                                           np.concatenate([[0], np.cumsum(h.sums['numHullVertices'][has])]), h.hullPoints,
                                           h.sums['hullArea2'][has].copy()))
    for k in ARRAYS:
        assert np.array_equal(getattr(again, k), getattr(h, k)), k
    for k in hc.SUMS:
        assert np.array_equal(again.sums[k], h.sums[k]), k


@pytest.mark.parametrize('four', [True, False], ids=['four', 'eight'])
@pytest.mark.parametrize('name', ['seg_final', 'random256'])
def test_real_rasters_against_the_model(name, four):
    check_raster(real_raster(name), four)


# ---- sources ----------------------------------------------------------------------------------------------------------
def test_sources():
    from pyshepseg_amd import neighbours, outlines
    seg = real_raster('seg_final')
    o = trace(seg, hulls=True)
    assert isinstance(o.hulls, outlines.SegmentHulls) and not o.hulls.timings['uploaded'] and 'hulls' in o.timings
    assert outlines.residentOutlineSerial() == o.residentSerial
    again = hulls(o)
    assert not again.timings['uploaded'] and again.timings['uploadDeviceMs'] == 0.0
    assert_equal(again, o.hulls)
    plain = trace(seg)                                  # the default: no hulls, and its rings replace o's in the context
    assert plain.hulls is None and 'hulls' not in plain.timings and outlines.residentOutlineSerial() == plain.residentSerial
    assert plain.residentSerial != o.residentSerial
    late = hulls(o)
    assert late.timings['uploaded']
    assert_equal(late, o.hulls)
    assert not hulls(plain).timings['uploaded']
    assert_same(late, hc.reference_hulls(o))
    # the recoded raster of a merge
    S = int(seg.max())
    nb = neighbours.findSegmentNeighbours(seg, True, maxSegId=S)
    m = neighbours.mergeSegments(nb, (np.arange(S + 1) % 3).astype(np.int64), segfile=seg)
    mo = trace(m, hulls=True)
    assert_same(mo.hulls, hc.reference_hulls(mo))
    assert_equal(hulls(by_hand(mo)), mo.hulls)


@functools.lru_cache(maxsize=None)
def two_ring_sets():
    """A: the junction trace of the worked example (ids 0 .. 3, 3 rings, 19 vertices), with its hulls; B: that of a
    staircase (ids 0 .. 2, 2 rings, 26 vertices), with its simplification at tolerance 1 (6 vertices remain).  Both from
    the sequential models, nothing from the GPU."""
    import types
    (a, b) = (sc.reference_junction_trace(oc.EXAMPLE), sc.reference_junction_trace(oc.staircase(6)))
    assert (a['maxSegId'], len(a['ringArea2']), len(a['vertices'])) == (3, 3, 19)
    assert (b['maxSegId'], len(b['ringArea2']), len(b['vertices'])) == (2, 2, 26)
    return (a, hc.reference_hulls(types.SimpleNamespace(**a)), b, sc.reference_simplify(b, 1.0))


@pytest.mark.parametrize('resident', ['neither', 'hulls', 'simplification'])
def test_the_hull_source_and_the_simplification_source_stay_independent(resident):
    """The hulls take rings A, then the simplification takes rings B, and only then both are built and downloaded: each
    must have worked on its own rings, whether both were uploaded or one of the two reads a trace's rings in place."""
    from pyshepseg_amd import _lib
    (a, hulls_a, b, simplified_b) = two_ring_sets()
    c = _lib.ctx()
    L = c._L

    def extent(r):
        (lo, hi) = (r['vertices'].min(axis=0), r['vertices'].max(axis=0))
        return [int(x) for x in (lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1])]

    def arrays(r, names, here):
        ptrs = [None if here else _lib.ptr(np.ascontiguousarray(r[k])) for k in names]
        return ptrs + [r['maxSegId'], len(r['ringArea2']), len(r['vertices']), None]
    names = ('ringOffsets', 'vertexOffsets', 'vertices', 'ringArea2')
    if resident == 'hulls':
        o = trace(oc.EXAMPLE, junctions=True)
        assert all(np.array_equal(getattr(o, k), a[k]) for k in names + ('junction',))
    c.check(L.shp_hull_source(c.handle, *arrays(a, names, resident == 'hulls')))
    if resident == 'simplification':                    # (its trace replaces no uploaded rings: the hulls' are in hl_*)
        o = trace(oc.staircase(6), junctions=True)
        assert all(np.array_equal(getattr(o, k), b[k]) for k in names + ('junction',))
    c.check(L.shp_simplify_source(c.handle, *arrays(b, names + ('junction',), resident == 'simplification')))
    counts = np.zeros(3, dtype=np.int64)
    c.check(L.shp_hull_build(c.handle, *extent(a), 1 if resident == 'hulls' else 0, _lib.ptr(counts), None))
    nh = int(counts[0])
    S = a['maxSegId']
    got = dict(hullOffsets=np.empty(S + 2, dtype=np.int64), hullPoints=np.empty((nh, 2), dtype=np.int64),
               hullReach=np.empty(nh, dtype=np.int64), hullArea2=np.empty(S + 1, dtype=np.int64),
               feretMax2=np.empty(S + 1, dtype=np.int64))
    c.check(L.shp_hull_download(c.handle, *[_lib.ptr(v) for v in got.values()]))
    for k in ARRAYS:
        assert got[k].shape == hulls_a[k].shape and np.array_equal(got[k], hulls_a[k]), k
    assert np.array_equal(got['hullOffsets'], hulls_a['hullOffsets'])
    assert np.array_equal(got['hullArea2'], hulls_a['sums']['hullArea2']) and np.array_equal(got['feretMax2'], hulls_a['sums']['feretMax2'])
    counts = np.zeros(10, dtype=np.int64)
    c.check(L.shp_simplify_build(c.handle, sc.tolerance2q(1.0), 0, *extent(b), _lib.ptr(counts), None))
    (nr2, nv2) = (int(counts[0]), int(counts[1]))
    assert (nr2, nv2) == (2, 6)
    S = b['maxSegId']
    got = dict(ringOffsets=np.empty(S + 2, dtype=np.int64), vertexOffsets=np.empty(nr2 + 1, dtype=np.int64),
               vertices=np.empty((nv2, 2), dtype=np.int64), ringArea2=np.empty(nr2, dtype=np.int64),
               sourceRing=np.empty(nr2, dtype=np.int64), keptVertex=np.empty(nv2, dtype=np.int64))
    c.check(L.shp_simplify_download(c.handle, *[_lib.ptr(v) for v in got.values()]))
    for k in got:
        assert got[k].shape == simplified_b[k].shape and np.array_equal(got[k], simplified_b[k]), k


# ---- entry points -----------------------------------------------------------------------------------------------------
def test_call_order_is_enforced_and_the_other_state_stays():
    from pyshepseg_amd import _lib, neighbours, shapes
    nb = neighbours.findSegmentNeighbours(nc.EXAMPLE, True)
    serial = neighbours.residentTableSerial()
    assert serial is not None and serial == nb.residentSerial
    c = _lib.ctx()
    L = c._L
    counts = np.full(3, 7, dtype=np.int64)
    out = [np.full(64, 7, dtype=np.int64) for _k in range(5)]

    def refused(rc, what):
        assert rc != 0
        assert what in L.shp_last_error(c.handle).decode()

    def source_call():
        return L.shp_hull_source(c.handle, None, None, None, None, 0, 0, 0, None)

    def build_call():
        return L.shp_hull_build(c.handle, 0, 0, 3, 3, 1, _lib.ptr(counts), None)

    def download_call():
        return L.shp_hull_download(c.handle, *[_lib.ptr(a) for a in out])
    c.check(L.shp_shape_begin(c.handle, 3, 0, 0))       # a shape table begun before, finished after the hulls
    (edges, bad) = (ctypes.c_int64(0), ctypes.c_uint32(0))
    c.check(L.shp_outline_edges_dev(c.handle, None, 0, 0, 0, 1, ctypes.byref(edges), ctypes.byref(bad)))
    refused(source_call(), 'shp_outline_trace must come first')
    refused(build_call(), 'shp_hull_source must come first')
    refused(download_call(), 'shp_hull_build must come first')
    assert counts.tolist() == [7, 7, 7] and out[0][0] == 7
    o = trace(oc.EXAMPLE)
    c.check(source_call())
    refused(download_call(), 'shp_hull_build must come first')
    refused(L.shp_hull_build(c.handle, 0, 0, 3, 3, 1, None, None), 'NULL')
    refused(L.shp_hull_build(c.handle, 0, 0, 2 ** 31, 1, 1, _lib.ptr(counts), None), 'spans')
    refused(L.shp_hull_build(c.handle, 0, 0, 2 ** 16 + 1, 2 ** 16, 1, _lib.ptr(counts), None), 'spans')
    c.check(build_call())
    assert counts.tolist() == [15, 15, 15]
    refused(L.shp_hull_download(c.handle, None, None, None, None, None), 'NULL')
    c.check(download_call())
    assert out[0][:5].tolist() == [0, 0, 5, 11, 15] and out[3][:4].tolist() == [0, 7, 10, 4] and out[4][:4].tolist() == [0, 8, 10, 5]
    # the outlines are still the trace's
    rings = [np.full(64, 7, dtype=np.int64) for _k in range(4)]
    c.check(L.shp_outline_download(c.handle, *[_lib.ptr(a) for a in rings]))
    assert rings[0][:5].tolist() == [0, 0, 1, 2, 3] and rings[3][:3].tolist() == oc.EXAMPLE_AREA2
    assert np.array_equal(rings[2][:36].reshape(18, 2), o.vertices)
    # a resident source whose outlines are replaced before the build
    c.check(source_call())
    c.check(L.shp_outline_edges_dev(c.handle, None, 0, 0, 0, 1, ctypes.byref(edges), ctypes.byref(bad)))
    refused(build_call(), 'the traced outlines have been replaced')
    refused(build_call(), 'shp_hull_source must come first')
    # uploaded arrays whose ends do not fit
    (ro, vo) = (o.ringOffsets, o.vertexOffsets.copy())
    vo[-1] = 17
    refused(L.shp_hull_source(c.handle, _lib.ptr(ro), _lib.ptr(vo), _lib.ptr(o.vertices), _lib.ptr(o.ringArea2), 3, 3, 18, None),
            'do not span')
    refused(L.shp_hull_source(c.handle, _lib.ptr(ro), None, _lib.ptr(o.vertices), _lib.ptr(o.ringArea2), 3, 3, 18, None), 'NULL')
    refused(L.shp_hull_source(c.handle, _lib.ptr(ro), _lib.ptr(vo), _lib.ptr(o.vertices), _lib.ptr(o.ringArea2), -1, 3, 18, None),
            'max_seg_id')
    # uploaded offsets that span their counts but descend once, per ring and per id: refused as shp_simplify_source
    # refuses them, and no rings are taken
    (vo, ro2) = (o.vertexOffsets.copy(), o.ringOffsets.copy())
    assert vo.tolist() == [0, 6, 14, 18] and ro2.tolist() == [0, 0, 1, 2, 3]
    vo[1] = 15
    ro2[2:4] = [2, 1]
    refused(L.shp_hull_source(c.handle, _lib.ptr(ro), _lib.ptr(vo), _lib.ptr(o.vertices), _lib.ptr(o.ringArea2), 3, 3, 18, None),
            'the vertex offsets do not ascend at ring 1')
    refused(build_call(), 'shp_hull_source must come first')
    refused(L.shp_hull_source(c.handle, _lib.ptr(ro2), _lib.ptr(o.vertexOffsets), _lib.ptr(o.vertices), _lib.ptr(o.ringArea2), 3, 3, 18,
                              None), 'the ring offsets do not ascend at id 2')
    refused(build_call(), 'shp_hull_source must come first')
    # o's rings are no longer resident (the calls above replaced them): the function sees that and uploads
    got = hulls(o)
    assert got.timings['uploaded']
    assert_same(got, hc.reference_hulls(o))
    (S, sbad) = (ctypes.c_uint32(0), ctypes.c_uint32(0))
    c.check(L.shp_shape_finish(c.handle, ctypes.byref(S), ctypes.byref(sbad), None))
    table = np.full((4, 11), 7, dtype=np.uint64)
    c.check(L.shp_shape_download(c.handle, _lib.ptr(table)))
    assert not table.any()
    assert neighbours.residentTableSerial() == serial
    red = neighbours.reduceOverNeighbours(nb, [(np.arange(4, dtype=np.float64), [('n', 'count')])])
    assert red['n'].tolist() == [0, 2, 2, 2] and not nb.reduceTimings['uploaded']
    assert shapes.calcSegmentShapes(oc.EXAMPLE).columns['perimeter'].tolist() == [0, 8, 10, 6]
    check_raster(oc.EXAMPLE)


def test_working_set_is_refused_before_it_is_allocated(monkeypatch):
    from pyshepseg_amd import _lib, outlines
    c = _lib.ctx()
    o = trace(oc.EXAMPLE)

    class Library(object):
        """the library, whose hull buffers would have to grow by a terabyte more"""
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            fn = getattr(c._L, name)

            def call(*args):
                self.calls.append(name)
                rc = fn(*args)
                if name == 'shp_hull_need':
                    args[5]._obj.value += 10 ** 12
                return rc
            return call

    class Ctx(object):
        def __init__(self):
            (self.handle, self.check, self._L) = (c.handle, c.check, Library())
    fake = Ctx()
    monkeypatch.setattr(_lib, 'ctx', lambda: fake)
    with pytest.raises(outlines.PyShepSegOutlinesError,
                       match=r'the hull arrays of 18 vertices, 3 rings and 4 ids need 1\d{12} bytes of device memory, \d+ are free'):
        outlines.calcSegmentHulls(o)
    assert fake._L.calls == ['shp_outline_serial', 'shp_hull_need']
    monkeypatch.undo()
    assert not hulls(o).timings['uploaded']             # nothing was launched or replaced: o is still resident


def test_a_trace_without_hulls_makes_the_calls_it_always_made(monkeypatch):
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
    outlines.traceSegmentOutlines(oc.EXAMPLE, maxSegId=3)
    assert [n for n in fake.calls if n.startswith(('shp_outline', 'shp_hull'))] == ['shp_outline_need', 'shp_outline_edges_dev', 'shp_outline_need',
                                                                       'shp_outline_trace', 'shp_outline_download']
    fake.calls = []
    outlines.traceSegmentOutlines(oc.EXAMPLE, maxSegId=3, hulls=True)
    assert [n for n in fake.calls if n.startswith('shp_hull')] == ['shp_hull_need', 'shp_hull_source', 'shp_hull_build', 'shp_hull_download']


def test_readme_example():
    """the README's lines: the hull columns into the column dictionary, one id's hull, the hulls with the trace"""
    from pyshepseg_amd import outlines, shapes
    seg = real_raster('mosaic')
    o = outlines.traceSegmentOutlines(seg, fourConnected=True)
    cols = dict(shapes.calcSegmentShapes(seg).columns)
    cols.update(o.columns)
    h = outlines.calcSegmentHulls(o)
    cols.update(h.columns)
    ring = h.hullOf(42)
    assert ring.shape == (cols['numHullVertices'][42], 2) and 0 < cols['solidity'][42] <= 1
    assert cols['feretMin'][42] <= cols['feretMax'][42] and cols['hullArea'][42] >= cols['area'][42]
    assert_equal(outlines.traceSegmentOutlines(seg, hulls=True).hulls, h)
