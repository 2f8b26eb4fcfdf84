"""Segment outlines as rings of vertices, traced on the GPU from the label raster.

Object-based work ends in polygons: a layer to lay over the imagery, to edit, to join to the per-segment columns.
``traceSegmentOutlines`` gives every segment's outline as vertex rings from the label raster alone (csrc/outline.h):
the boundary sides that shapes.calcSegmentShapes counts as ``perimeter`` are put in order here.

Definitions.  Pixel (y, x) covers [y, y + 1] x [x, x + 1]; corners are integer (row, col) pairs; label 0 is no segment.
A side of a pixel of id A is an edge of A when the label across it differs from A: another id, label 0 and outside the
raster all count.  Edges are directed with A's pixel on the right of travel:

    side 0 (N): (y, x) -> (y, x + 1)            side 2 (S): (y + 1, x + 1) -> (y + 1, x)
    side 1 (E): (y, x + 1) -> (y + 1, x + 1)    side 3 (W): (y + 1, x) -> (y, x)

An edge's key is (y, x, side).  An edge arrives at its end corner; with R = the pixel right-ahead is A and L = the pixel
left-ahead is A its successor is: not R, the next side of the same pixel (a right turn); R and not L, the same side of
the pixel right-ahead (straight on); R and L, side - 1 of the pixel left-ahead (a left turn).  At a saddle (not R, L: A
touches itself diagonally) ``fourConnected=True`` turns right and the two pixels stay apart, ``fourConnected=False``
turns left and they are joined.  A turn edge is an edge whose predecessor has another side number; its start corner
is a vertex.  A ring is one cycle of the successor map: the start corners of its turn edges in cycle order, beginning
with the turn edge of the smallest key.  ``ringArea2`` = sum(c_i r_(i+1) - c_(i+1) r_i) is positive for an outer ring
(clockwise on screen) and negative for a hole; half its magnitude is the pixels enclosed.  Rings are ordered by (id,
key of the first turn edge), so every id's first ring is an outer ring.

A ring may touch itself at a saddle corner (with ``fourConnected=False`` an outer ring passes such a corner twice, with
``fourConnected=True`` a hole may), as the rings of ``gdal_polygonize`` do: the rings are valid boundaries of the pixel
sets, not always simple polygons in the OGC sense.

The labels are whole in HBM for this function: a host array or ``.npy`` file is uploaded once, resident labels are
read in place.  The working set is 9 bytes a pixel (labels included), 37 bytes an edge, 16 a vertex and about 52 a
ring; when the free HBM does not hold it the call raises before anything is allocated.  There is no CPU fallback.
Streaming in row blocks and a multi-rank form do not exist yet.

``calcSegmentHulls`` takes every segment's convex hull from the rings (csrc/hull.h), in place while they are still in
HBM, and with it the hull-based shape attributes: ``solidity``, ``convexity``, ``feretMin``, ``feretMax``.

``simplifySegmentOutlines`` is a topology-aware Douglas-Peucker simplification of all rings (csrc/simplify.h).  Labels
outside the raster read as 0; of the four pixels a b / c d round a corner the pairs (a, b), (b, d), (c, d), (a, c) that
differ number the corner's degree (0, 2, 3 or 4), and a corner of degree >= 3 is a junction, whatever ``fourConnected``
(the two-label saddle A B / B A has degree 4).  The junction trace, ``traceSegmentOutlines(..., junctions=True)``, makes
a vertex of every edge that is a turn edge or whose start corner is a junction -- the ring that runs straight through a
T-junction gets a collinear vertex there -- starts a ring at its vertex edge of the smallest key, and flags the junction
vertices in ``junction``; ``ringArea2``, ``numParts``, ``numHoles``, ``holeArea`` and the hulls are the plain trace's.
A ring's anchors are its junction vertices (a ring without any: its vertex of the smallest (row, col)), an arc runs from
one anchor to the next in ring order, cyclically, and may be closed.  With T = floor(tolerance^2 * 65536): both ends of
an arc are kept; between kept points a and b, m(q) = |(b - a) x (q - a)| if a != b and |q - a|^2 if a = b; the candidate
is the point of the largest m, ties to the smallest (row, col); it exceeds the tolerance when m^2 * 65536 > T * |b - a|^2
(a != b) or m * 65536 > T (a = b), in 128-bit integers; a candidate that exceeds is kept and both halves are treated the
same way, otherwise nothing between a and b is kept.  The two rings that share an arc run it in opposite directions and
every quantity is symmetric, so both keep the same corners: along a shared border neighbours keep identical vertices.
Arcs may still cross each other at large tolerances; that is not checked.
"""
import ctypes
import json
import time

import numpy

from . import _lib
from . import labelsource


class PyShepSegOutlinesError(Exception):
    pass


COLUMNS = ('numParts', 'numHoles', 'numVertices', 'holeArea')
# pixels, and edges, one call can take (csrc/outline.h: OL_MAX_ITEMS)
MAX_ITEMS = 2 ** 32 - 8192


def _segmentSums(values, offsets):
    """sum of values[offsets[i]:offsets[i + 1]] for every i, int64"""
    cs = numpy.zeros(len(values) + 1, dtype=numpy.int64)
    numpy.cumsum(values, out=cs[1:])
    return cs[offsets[1:]] - cs[offsets[:-1]]


def columnsFromRings(ringOffsets, vertexOffsets, ringArea2):
    """The int64 columns COLUMNS, one row per id: ``numParts`` the id's outer rings, ``numHoles`` its holes,
    ``numVertices`` the vertices of all its rings, ``holeArea`` the pixels its holes enclose."""
    outer = (ringArea2 > 0).astype(numpy.int64)
    hole = (ringArea2 < 0).astype(numpy.int64)
    return {'numParts': _segmentSums(outer, ringOffsets),
            'numHoles': _segmentSums(hole, ringOffsets),
            'numVertices': _segmentSums(numpy.diff(vertexOffsets), ringOffsets),
            'holeArea': _segmentSums(numpy.where(ringArea2 < 0, -ringArea2, 0) // 2, ringOffsets)}


def _checkSegId(segId, maxSegId):
    if isinstance(segId, (bool, numpy.bool_)) or not isinstance(segId, (int, numpy.integer)) or not 0 <= segId <= maxSegId:
        raise PyShepSegOutlinesError("segment id must be an integer 0 .. {} (got {!r})".format(maxSegId, segId))


class SegmentOutlines(object):
    """The result of traceSegmentOutlines, for the ids 0 .. ``maxSegId`` (S = maxSegId + 1 rows).

    ``ringOffsets``: int64, S + 1 long, the rings of id i are ``ringOffsets[i]:ringOffsets[i + 1]``;
    ``vertexOffsets``: int64, rings + 1 long; ``vertices``: int64 (n, 2) as (row, col), ``origin`` added;
    ``ringArea2``: int64, positive for outer rings, negative for holes; ``columns``: the int64 columns COLUMNS as the
    statistics' column dictionaries hold them; ``rounds``: pointer-doubling rounds run; ``edges``: boundary sides;
    ``timings``: seconds per step; ``deviceMs``: GPU time of the kernels, ``deviceStepsMs`` its split; ``junction``:
    uint8, one entry per vertex, 1 where the vertex's corner is a junction (a junction trace), None for a plain trace."""
    def __init__(self, maxSegId, ringOffsets, vertexOffsets, vertices, ringArea2, origin=(0, 0), fourConnected=True,
                 rounds=0, edges=None, timings=None, deviceMs=None, deviceStepsMs=None, junction=None):
        self.maxSegId = maxSegId
        self.ringOffsets = ringOffsets
        self.vertexOffsets = vertexOffsets
        self.vertices = vertices
        self.ringArea2 = ringArea2
        self.origin = origin
        self.fourConnected = fourConnected
        self.rounds = rounds
        self.edges = edges
        self.timings = timings if timings is not None else {}
        self.deviceMs = deviceMs
        self.deviceStepsMs = deviceStepsMs if deviceStepsMs is not None else {}
        self.columns = columnsFromRings(ringOffsets, vertexOffsets, ringArea2)
        # which outlines of which context these are (residentOutlineSerial); None for rings built by hand
        self.residentSerial = None
        self._residentCtx = None
        self.hulls = None           # a SegmentHulls after traceSegmentOutlines(hulls=True)
        self.junction = junction    # uint8, a flag per vertex, after traceSegmentOutlines(junctions=True); None for a plain trace
        self.simplified = None      # a SimplifiedOutlines after traceSegmentOutlines(simplify=tolerance)

    def _ringRange(self, segId):
        _checkSegId(segId, self.maxSegId)
        return range(int(self.ringOffsets[segId]), int(self.ringOffsets[segId + 1]))

    def ring(self, r):
        return self.vertices[int(self.vertexOffsets[r]):int(self.vertexOffsets[r + 1])]

    def ringsOf(self, segId):
        """the id's rings, outer rings and holes in ring order: a list of (k, 2) arrays (views of ``vertices``)"""
        return [self.ring(r) for r in self._ringRange(segId)]

    def _holeShells(self, segId):
        """{hole: shell}, both ring numbers, for the holes of the id"""
        rings = list(self._ringRange(segId))
        shells = [r for r in rings if self.ringArea2[r] > 0]
        owner = {}
        for r in rings:
            if self.ringArea2[r] > 0:
                continue
            if len(shells) == 1:
                owner[r] = shells[0]
                continue
            v = self.ring(r)
            d = numpy.sign(v[1] - v[0])                 # direction of travel (drow, dcol); the pixel lies to its right
            centre = v[0] + 0.5 * d + 0.5 * numpy.array([d[1], -d[0]])
            inside = [s for s in shells if _contains(self.ring(s), centre)]
            if not inside:
                raise PyShepSegOutlinesError("a hole of segment {} lies in none of its outer rings".format(segId))
            owner[r] = min(inside, key=lambda s: self.ringArea2[s])
        return owner

    def polygonsOf(self, segId):
        """The id's polygons: a list of [shell, hole, ...], the shells in ring order and every hole with its shell.

        An id with one outer ring owns all its holes.  With several, a hole goes to the enclosing shell of the
        smallest area, decided on the host: the centre of the pixel of the hole's first edge (the pixel right-ahead of
        vertex 0 heading to vertex 1, a pixel of the id) lies strictly inside every shell that encloses the hole."""
        rings = list(self._ringRange(segId))
        shells = [r for r in rings if self.ringArea2[r] > 0]
        owner = self._holeShells(segId)
        polys = {r: [self.ring(r)] for r in shells}
        for r in rings:
            if r in owner:
                polys[owner[r]].append(self.ring(r))
        return [polys[r] for r in shells]


def _contains(ring, point):
    """point (row, col), with half-integer coordinates, strictly inside the rectilinear ring: a ray towards
    increasing col crosses an odd number of its vertical segments"""
    nxt = numpy.roll(ring, -1, axis=0)
    vertical = ring[:, 1] == nxt[:, 1]
    lo = numpy.minimum(ring[:, 0], nxt[:, 0])
    hi = numpy.maximum(ring[:, 0], nxt[:, 0])
    crossed = vertical & (ring[:, 1] > point[1]) & (lo < point[0]) & (point[0] < hi)
    return bool(numpy.count_nonzero(crossed) & 1)


def _xy(ring, transform):
    """a ring's (x, y) pairs, closed: without a transform x = col and y = row, with a GDAL six-tuple applied to (col,
    row)"""
    col = ring[:, 1].astype(numpy.float64)
    row = ring[:, 0].astype(numpy.float64)
    if transform is None:
        (x, y) = (col, row)
    else:
        t = [float(v) for v in transform]
        if len(t) != 6:
            raise PyShepSegOutlinesError("transform must be a GDAL geotransform of six numbers")
        x = t[0] + col * t[1] + row * t[2]
        y = t[3] + col * t[4] + row * t[5]
    pts = [[float(a), float(b)] for (a, b) in zip(x.tolist(), y.tolist())]
    return pts + pts[:1]


def _num(v):
    return repr(int(v)) if float(v).is_integer() else repr(float(v))


def toWKT(o, segId, transform=None):
    """The id's outline as a WKT MULTIPOLYGON (``MULTIPOLYGON EMPTY`` for an id without pixels), rings closed.
    ``transform`` is a GDAL six-tuple applied to (col, row); without one x = col and y = row.

    Plain Python, for looking at results and exporting chosen ids; not meant for millions of features."""
    polys = o.polygonsOf(segId)
    if not polys:
        return 'MULTIPOLYGON EMPTY'
    return 'MULTIPOLYGON (' + ', '.join(
        '(' + ', '.join('(' + ', '.join(_num(x) + ' ' + _num(y) for (x, y) in _xy(ring, transform)) + ')' for ring in poly) + ')'
        for poly in polys) + ')'


def writeGeoJSON(o, path, ids=None, transform=None, columns=None):
    """Write a GeoJSON FeatureCollection of MultiPolygons to ``path``: one feature per id of ``ids`` (default: every
    id with a ring), with the property ``segId`` and one property per entry of ``columns`` (a dictionary of
    per-segment columns, maxSegId + 1 rows each).  ``transform`` as in toWKT.  Returns the number of features.

    Plain Python, for looking at results and exporting chosen ids; not meant for millions of features."""
    if ids is None:
        ids = numpy.flatnonzero(numpy.diff(o.ringOffsets) > 0)
    columns = dict(columns) if columns is not None else {}
    for (name, col) in columns.items():
        if len(col) != o.maxSegId + 1:
            raise PyShepSegOutlinesError("column {!r} has {} rows, not maxSegId + 1 = {}".format(name, len(col), o.maxSegId + 1))
    features = []
    for i in ids:
        i = int(i)
        props = {'segId': i}
        for (name, col) in columns.items():
            v = col[i]
            props[name] = v.item() if isinstance(v, numpy.generic) else v
        coords = [[_xy(ring, transform) for ring in poly] for poly in o.polygonsOf(i)]
        features.append({'type': 'Feature', 'properties': props, 'geometry': {'type': 'MultiPolygon', 'coordinates': coords}})
    with open(path, 'w') as f:
        json.dump({'type': 'FeatureCollection', 'features': features}, f)
    return len(features)


def _checkArgs(segfile, maxSegId, origin):
    """(the labelsource.Labels of the raster, (row0, col0)): everything that can be refused before the GPU is touched; the
    raster, ``maxSegId`` and ``origin`` as shapes.calcSegmentShapes takes them"""
    Err = PyShepSegOutlinesError
    labels = labelsource.resolve(segfile, maxSegId, Err, merged=True, hint=True)
    origin = labelsource.checkOrigin(origin, labels.nrows, labels.ncols, Err)
    if labels.nrows * labels.ncols > MAX_ITEMS:
        raise Err("a raster of {} pixels: more than the {} one call can take".format(labels.nrows * labels.ncols, MAX_ITEMS))
    return (labels, origin)


def traceSegmentOutlines(segfile, fourConnected=True, maxSegId=None, origin=(0, 0), hulls=False, junctions=False, simplify=None):
    """
    The outline of every segment of a label raster as vertex rings, on the GPU: a SegmentOutlines.  With ``hulls=True``
    its ``hulls`` is the SegmentHulls of calcSegmentHulls, taken while the rings are still in HBM.

    ``junctions=True`` is the junction trace (module docstring): every corner where three or more segments meet is a
    vertex of all rings through it, and ``junction`` flags those vertices.  ``simplify=tolerance`` implies it and sets
    ``simplified`` to the SimplifiedOutlines of simplifySegmentOutlines, taken while the rings are still in HBM.

    ``segfile`` is what shapes.calcSegmentShapes takes -- a 2-D uint32 array, a ``.npy`` path, a
    TiledSegmentationResult (its ``segimg``), a result whose labels are in HBM (``outDev``, read in place) or a
    MergedSegments (its ``outDev`` if it has one, else its ``segimg``).  A host raster is uploaded once, whole.

    ``fourConnected`` decides the saddle corners (module docstring).  ``maxSegId`` is the last row of every column and
    of ``ringOffsets``; None takes the ``maxSegId`` of a result object that carries one, otherwise the largest label,
    found by a reduction on the GPU.  A label above a given ``maxSegId`` raises PyShepSegOutlinesError with the largest
    such label.  ``origin`` = (row0, col0), non-negative integers, is added to the vertex coordinates and changes
    nothing else.

    The raster has at most 2^32 - 8192 pixels and as many edges, and the working set (module docstring) must fit the
    free HBM: otherwise PyShepSegOutlinesError names the bytes needed, before anything is allocated.
    """
    (labels, origin) = _checkArgs(segfile, maxSegId, origin)
    (nrows, ncols, maxSegId) = (labels.nrows, labels.ncols, labels.maxSegId)
    if simplify is not None:
        tolerance2q(simplify)
        junctions = True
    t0 = time.perf_counter()
    c = _lib.ctx()
    L = c._L
    if hulls or simplify is not None:
        _outlineSerial(c)
    npix = nrows * ncols
    timings = {}
    (need, free) = (ctypes.c_int64(0), ctypes.c_int64(0))
    deviceMs = 0.0
    with labelsource.LabelSource(c, labels) as src:
        c.check(L.shp_outline_need(c.handle, npix, -1, ctypes.byref(need), ctypes.byref(free)))
        want = need.value + (4 * npix if labels.devSeg is None else 0)
        if want > free.value:
            raise PyShepSegOutlinesError("the labels and per-pixel arrays of {} x {} pixels need {} bytes of device memory, {} are "
                                         "free".format(nrows, ncols, want, free.value))
        dseg = src.whole()
        timings['upload'] = time.perf_counter() - t0
        if maxSegId is None:
            t1 = time.perf_counter()
            (maxSegId, deviceMs) = src.labelMax(PyShepSegOutlinesError)
            timings['labelMax'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        (edges, bad) = (ctypes.c_int64(0), ctypes.c_uint32(0))
        serial = c._outlineEdgeCalls = getattr(c, '_outlineEdgeCalls', 0) + 1
        c.check(L.shp_outline_edges_dev(c.handle, dseg, nrows, ncols, maxSegId, int(bool(fourConnected)), ctypes.byref(edges),
                                        ctypes.byref(bad)))
        if bad.value:
            raise PyShepSegOutlinesError("segment id {} is above maxSegId {}".format(bad.value, maxSegId))
        if edges.value > MAX_ITEMS:
            raise PyShepSegOutlinesError("{} edges: more than the {} one call can take".format(edges.value, MAX_ITEMS))
        if junctions:
            c.check(L.shp_outline_junctions(c.handle, 1))
        c.check(L.shp_outline_need(c.handle, npix, edges.value, ctypes.byref(need), ctypes.byref(free)))
        if need.value > free.value:
            raise PyShepSegOutlinesError("the per-edge arrays of {} edges need {} bytes of device memory, {} are "
                                         "free".format(edges.value, need.value, free.value))
        timings['edges'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        counts = numpy.zeros(3, dtype=numpy.int64)
        steps = numpy.zeros(4, dtype=numpy.float64)
        c.check(L.shp_outline_trace(c.handle, origin[0], origin[1], _lib.ptr(counts), _lib.ptr(steps)))
        timings['trace'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        (nrings, nverts, rounds) = (int(v) for v in counts)
        ringOffsets = numpy.empty(maxSegId + 2, dtype=numpy.int64)
        vertexOffsets = numpy.empty(nrings + 1, dtype=numpy.int64)
        vertices = numpy.empty((nverts, 2), dtype=numpy.int64)
        ringArea2 = numpy.empty(nrings, dtype=numpy.int64)
        c.check(L.shp_outline_download(c.handle, _lib.ptr(ringOffsets), _lib.ptr(vertexOffsets), _lib.ptr(vertices),
                                       _lib.ptr(ringArea2)))
        junction = None
        if junctions:
            junction = numpy.empty(nverts, dtype=numpy.uint8)
            c.check(L.shp_outline_download_junction(c.handle, _lib.ptr(junction)))
        timings['download'] = time.perf_counter() - t1
    deviceStepsMs = dict(zip(('edges', 'successors', 'rounds', 'rings'), steps.tolist()))
    deviceMs += float(steps.sum())
    t1 = time.perf_counter()
    out = SegmentOutlines(maxSegId, ringOffsets, vertexOffsets, vertices, ringArea2, origin=origin,
                          fourConnected=bool(fourConnected), rounds=rounds, edges=int(edges.value), deviceMs=deviceMs,
                          deviceStepsMs=deviceStepsMs, junction=junction)
    timings['columns'] = time.perf_counter() - t1
    (out.residentSerial, out._residentCtx) = (serial, c.handle.value)
    if hulls:
        t1 = time.perf_counter()
        out.hulls = calcSegmentHulls(out)
        timings['hulls'] = time.perf_counter() - t1
    if simplify is not None:
        t1 = time.perf_counter()
        out.simplified = simplifySegmentOutlines(out, simplify)
        timings['simplify'] = time.perf_counter() - t1
    timings['total'] = time.perf_counter() - t0
    out.timings = timings
    return out


# ---- convex hulls of the rings: solidity and Feret diameters (csrc/hull.h) ----------------------------------------------
HULL_SUMS = ('numHullVertices', 'hullArea2', 'feretMax2')
HULL_DERIVED = ('hullArea', 'solidity', 'hullPerimeter', 'convexity', 'feretMax', 'feretMin', 'feretRatio')
HULL_STEPS = ('candidates', 'order', 'chains', 'points', 'reach')


def _outlineSerial(c):
    """The serial of the traced outlines context ``c`` holds on the device, None without any.  The serial is the count
    of the context's shp_outline_edges_dev calls at the trace; traceSegmentOutlines counts its own calls on the context
    object instead of asking (a trace makes the calls it always made), and every question brings that count up to the
    library's, so a count that calls from elsewhere have left behind can only make outlines look replaced."""
    (calls, serial) = (ctypes.c_uint64(0), ctypes.c_uint64(0))
    c.check(c._L.shp_outline_serial(c.handle, ctypes.byref(calls), ctypes.byref(serial)))
    c._outlineEdgeCalls = calls.value
    return serial.value if serial.value else None


def residentOutlineSerial():
    """The serial of the traced outlines the calling thread's context holds on the device, None without any: a
    SegmentOutlines whose ``residentSerial`` it is still has its rings in HBM, and calcSegmentHulls reads them there."""
    return _outlineSerial(_lib.ctx())


def _perId(values, offsets, ufunc, empty):
    """ufunc.reduce over values[offsets[i]:offsets[i + 1]] for every i, ``empty`` where the range is empty"""
    out = numpy.full(len(offsets) - 1, empty, dtype=numpy.float64)
    has = numpy.flatnonzero(numpy.diff(offsets) > 0)
    if len(has):
        out[has] = ufunc.reduceat(values, offsets[:-1][has])
    return out


def hullColumnsFromSums(sums, hullOffsets, hullPoints, hullReach, ringArea2Sum, perimeter, missing=-9999):
    """
    The float64 columns HULL_DERIVED from the integers of the GPU, as a dictionary: ``sums`` the int64 columns HULL_SUMS,
    the hulls' offsets, points and per-edge reach, ``ringArea2Sum`` the sum of the id's ringArea2 (twice its pixels)
    and ``perimeter`` the sum of its rings' lengths (the shape table's ``perimeter``).

    ``hullArea`` = hullArea2 / 2; ``solidity`` = ringArea2Sum / hullArea2; ``hullPerimeter`` = the sum of the hull
    edges' lengths; ``convexity`` = hullPerimeter / perimeter; ``feretMax`` = sqrt(feretMax2); ``feretMin`` = the
    minimum over the hull's edges of hullReach / sqrt(squared edge length), the width between the edge's line and the
    parallel support line; ``feretRatio`` = feretMin / feretMax.  Rows without hull points, and ratios whose
    denominator is 0, hold ``missing``.

    The minimum over the edges is taken here, in float64, and not on the GPU: comparing reach^2 / length^2 of two
    edges exactly takes more than 128 bits at the coordinate limits, while every edge's reach and squared length are
    exact integers and the hulls have far fewer points than the rings.
    """
    n = len(hullOffsets) - 1
    out = {name: numpy.full(n, float(missing), dtype=numpy.float64) for name in HULL_DERIVED}
    has = numpy.asarray(sums['numHullVertices']) > 0
    if not has.any():
        return out
    ho = numpy.asarray(hullOffsets)
    pts = numpy.asarray(hullPoints)
    nxt = numpy.arange(len(pts), dtype=numpy.int64) + 1
    idOf = numpy.repeat(numpy.arange(n), numpy.diff(ho))
    last = nxt == ho[1:][idOf]
    nxt[last] = ho[:-1][idOf][last]
    d = pts[nxt] - pts
    len2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]            # exact: below 2^63 within the limits
    length = numpy.sqrt(len2.astype(numpy.float64))
    with numpy.errstate(divide='ignore', invalid='ignore'):
        width = numpy.where(len2 > 0, numpy.asarray(hullReach).astype(numpy.float64) / length, 0.0)
    a2 = numpy.asarray(sums['hullArea2']).astype(numpy.float64)
    f2 = numpy.asarray(sums['feretMax2']).astype(numpy.float64)
    hullPerimeter = _perId(length, ho, numpy.add, 0.0)
    feretMin = _perId(width, ho, numpy.minimum, 0.0)
    feretMax = numpy.sqrt(f2)
    per = numpy.asarray(perimeter).astype(numpy.float64)
    out['hullArea'][has] = a2[has] / 2.0
    out['hullPerimeter'][has] = hullPerimeter[has]
    out['feretMax'][has] = feretMax[has]
    out['feretMin'][has] = feretMin[has]
    for (name, num, den) in (('solidity', numpy.asarray(ringArea2Sum).astype(numpy.float64), a2), ('convexity', hullPerimeter, per),
                             ('feretRatio', feretMin, feretMax)):
        ok = has & (den > 0)
        out[name][ok] = num[ok] / den[ok]
    return out


class SegmentHulls(object):
    """The result of calcSegmentHulls, for the ids 0 .. ``maxSegId`` (S = maxSegId + 1 rows).

    ``hullOffsets``: int64, S + 1 long, the hull of id i is ``hullPoints[hullOffsets[i]:hullOffsets[i + 1]]`` (empty
    for an id without rings); ``hullPoints``: int64 (n, 2) as (row, col), the outlines' origin included: the strict
    convex hull of all vertices of the id's rings, without repeated points or three consecutive collinear points,
    oriented like an outer ring and starting at the hull vertex of the smallest (row, col); ``hullReach``: int64 (n),
    for the hull edge from point k to its successor the largest cross product with the hull's points; ``sums``: the
    int64 columns HULL_SUMS (all 0 for an id without rings); ``columns``: those and the float64 columns HULL_DERIVED of
    hullColumnsFromSums; ``timings``: seconds per step, ``timings['uploaded']`` whether the rings had to go up;
    ``deviceMs``: GPU time of the kernels, ``deviceStepsMs`` its split into HULL_STEPS."""
    def __init__(self, maxSegId, hullOffsets, hullPoints, hullReach, sums, columns, timings=None, deviceMs=None,
                 deviceStepsMs=None, candidates=None, kept=None):
        self.maxSegId = maxSegId
        self.hullOffsets = hullOffsets
        self.hullPoints = hullPoints
        self.hullReach = hullReach
        self.sums = sums
        self.columns = columns
        self.timings = timings if timings is not None else {}
        self.deviceMs = deviceMs
        self.deviceStepsMs = deviceStepsMs if deviceStepsMs is not None else {}
        self.candidates = candidates
        self.kept = kept

    def hullOf(self, segId):
        """the id's hull: a (k, 2) array (a view of ``hullPoints``)"""
        _checkSegId(segId, self.maxSegId)
        return self.hullPoints[int(self.hullOffsets[segId]):int(self.hullOffsets[segId + 1])]


def _ringLengths(vertexOffsets, vertices):
    """the length of every ring, float64 (whole numbers for rectilinear rings)"""
    vo = numpy.asarray(vertexOffsets)
    v = numpy.asarray(vertices)
    if len(v) == 0:
        return numpy.zeros(len(vo) - 1, dtype=numpy.float64)
    d = numpy.empty(v.shape, dtype=numpy.float64)       # from every vertex to the next one, of a ring's last to its first
    d[:-1] = v[1:] - v[:-1]
    has = numpy.flatnonzero(numpy.diff(vo) > 0)
    d[vo[1:][has] - 1] = v[vo[:-1][has]] - v[vo[1:][has] - 1]
    return _perId(numpy.hypot(d[:, 0], d[:, 1]), vo, numpy.add, 0.0)


def _checkRings(o):
    """(ringOffsets, vertexOffsets, vertices, ringArea2 as contiguous int64 arrays, (row base, col base), (H, W)):
    everything that can be refused before the GPU is touched"""
    S = o.maxSegId
    if isinstance(S, (bool, numpy.bool_)) or not isinstance(S, (int, numpy.integer)) or not 0 <= S < 0xFFFFFFFE:
        raise PyShepSegOutlinesError("maxSegId must be an integer 0 .. 2^32 - 3 (got {!r})".format(S))
    arrays = []
    for (name, ndim) in (('ringOffsets', 1), ('vertexOffsets', 1), ('vertices', 2), ('ringArea2', 1)):
        a = numpy.asarray(getattr(o, name))
        if a.dtype != numpy.int64 or a.ndim != ndim:
            raise PyShepSegOutlinesError("{} must be an int64 array of {} dimension(s)".format(name, ndim))
        arrays.append(numpy.ascontiguousarray(a))
    (ro, vo, v, a2) = arrays
    if v.shape[1:] != (2,):
        raise PyShepSegOutlinesError("vertices must have the shape (n, 2)")
    if len(ro) != S + 2 or len(vo) != len(a2) + 1:
        raise PyShepSegOutlinesError("ringOffsets must have maxSegId + 2 entries and vertexOffsets one more than ringArea2")
    for (name, off, n) in (('ringOffsets', ro, len(a2)), ('vertexOffsets', vo, len(v))):
        if off[0] != 0 or off[-1] != n or numpy.any(numpy.diff(off) < 0):
            raise PyShepSegOutlinesError("{} must ascend from 0 to {}".format(name, n))
    if len(v) > MAX_ITEMS or len(a2) > MAX_ITEMS:
        raise PyShepSegOutlinesError("{} vertices in {} rings: more than the {} one call can take".format(len(v), len(a2), MAX_ITEMS))
    (base, span) = ((0, 0), (0, 0))
    if len(v):
        lo = [int(x) for x in v.min(axis=0)]
        hi = [int(x) for x in v.max(axis=0)]
        if min(lo) < -2 ** 62 or max(hi) > 2 ** 62:
            raise PyShepSegOutlinesError("vertex coordinates beyond +-2^62")
        (H, W) = (hi[0] - lo[0], hi[1] - lo[1])
        if H * W > 2 ** 32 or max(H, W) >= 2 ** 31:
            raise PyShepSegOutlinesError("the vertices span {} rows and {} columns: the hulls take spans H, W with H W <= 2^32 and "
                                         "max(H, W) < 2^31".format(H, W))
        (base, span) = ((lo[0], lo[1]), (H, W))
    return (ro, vo, v, a2, base, span)


def _takeRings(c, o, arrays, need, source, word, timings, t0):
    """The rings a hull call or a simplification works on, taken on context ``c``: whether ``o``'s rings are still the
    ones its trace left in HBM (they are then read in place, and nothing goes up).  ``arrays``: the checked ringOffsets,
    vertexOffsets, vertices, ringArea2 (and the flags, where ``source`` takes them), which are uploaded otherwise;
    ``need`` and ``source``: the library's pair of calls; ``word``: what the refusal calls the arrays.  Fills
    ``timings['need']`` (from ``t0``: with the caller's checks, two passes over the vertices for their extent),
    ``'upload'``, ``'uploaded'`` and ``'uploadDeviceMs'``."""
    (S, nrings, nverts) = (int(o.maxSegId), len(arrays[3]), len(arrays[2]))
    serial = _outlineSerial(c)
    resident = (serial is not None and getattr(o, 'residentSerial', None) == serial and
                getattr(o, '_residentCtx', None) == c.handle.value)
    (bytesNeeded, free) = (ctypes.c_int64(0), ctypes.c_int64(0))
    c.check(need(c.handle, nverts, nrings, S, 0 if resident else 1, ctypes.byref(bytesNeeded), ctypes.byref(free)))
    if bytesNeeded.value > free.value:
        raise PyShepSegOutlinesError("the {} arrays of {} vertices, {} rings and {} ids need {} bytes of device memory, {} are "
                                     "free".format(word, nverts, nrings, S + 1, bytesNeeded.value, free.value))
    timings['need'] = time.perf_counter() - t0
    t1 = time.perf_counter()
    ms = ctypes.c_double(0)
    ptrs = [None if resident else _lib.ptr(a) for a in arrays]
    c.check(source(c.handle, *ptrs, S, nrings, nverts, ctypes.byref(ms)))
    timings['upload'] = time.perf_counter() - t1
    timings['uploaded'] = not resident
    timings['uploadDeviceMs'] = ms.value
    return resident


def calcSegmentHulls(o, missing=-9999):
    """
    The convex hull of every segment of a SegmentOutlines ``o``, on the GPU: a SegmentHulls, with the hull-based shape
    attributes ``solidity`` (area over hull area: ragged against smooth, where compactness cannot tell),
    ``convexity``, and the Feret diameters ``feretMin``, ``feretMax`` (width and length independent of the axes).

    If ``o``'s rings are still the ones its trace left in HBM (``o.residentSerial`` is residentOutlineSerial() of the
    same context) they are read in place; otherwise ``vertices``, ``vertexOffsets``, ``ringOffsets`` and ``ringArea2``
    are uploaded once, which also allows rings that no raster produced (any SegmentOutlines built by hand).  All parts
    of an id form one hull, and holes cannot matter.  Everything up to the final square roots is integer arithmetic on
    the GPU (csrc/hull.h); ``missing`` fills the float columns of ids without rings.

    The minimum width is the one comparison left to the host: comparing reach^2 / length^2 of two hull edges exactly
    takes more than 128 bits at the coordinate limits, so the GPU returns every hull edge's exact ``hullReach`` and
    hullColumnsFromSums takes the minimum of reach / length in float64 over the hull, which has far fewer points than
    the rings.

    Limits, checked before the GPU is touched: with H and W the row and column spans of all vertices, H W <= 2^32 and
    max(H, W) < 2^31 (every cross product then stays within 2^33, every squared distance fits int64); traced outlines
    always satisfy this.  The working set is sized from the vertices, rings and ids alone, never from a bounding box;
    when the free HBM does not hold it PyShepSegOutlinesError names the bytes before anything is allocated.
    """
    t0 = time.perf_counter()
    (ro, vo, v, a2, base, span) = _checkRings(o)
    S = int(o.maxSegId)
    c = _lib.ctx()
    L = c._L
    timings = {}
    resident = _takeRings(c, o, (ro, vo, v, a2), L.shp_hull_need, L.shp_hull_source, 'hull', timings, t0)
    t1 = time.perf_counter()
    counts = numpy.zeros(3, dtype=numpy.int64)
    steps = numpy.zeros(5, dtype=numpy.float64)
    # only the trace's own rings are known to have their hull vertices among the convex corners of the outer rings
    c.check(L.shp_hull_build(c.handle, base[0], base[1], span[0], span[1], 1 if resident else 0, _lib.ptr(counts), _lib.ptr(steps)))
    timings['build'] = time.perf_counter() - t1
    t1 = time.perf_counter()
    nh = int(counts[0])
    hullOffsets = numpy.empty(S + 2, dtype=numpy.int64)
    hullPoints = numpy.empty((nh, 2), dtype=numpy.int64)
    hullReach = numpy.empty(nh, dtype=numpy.int64)
    hullArea2 = numpy.empty(S + 1, dtype=numpy.int64)
    feretMax2 = numpy.empty(S + 1, dtype=numpy.int64)
    c.check(L.shp_hull_download(c.handle, _lib.ptr(hullOffsets), _lib.ptr(hullPoints), _lib.ptr(hullReach), _lib.ptr(hullArea2),
                                _lib.ptr(feretMax2)))
    timings['download'] = time.perf_counter() - t1
    t1 = time.perf_counter()
    sums = {'numHullVertices': numpy.diff(hullOffsets), 'hullArea2': hullArea2, 'feretMax2': feretMax2}
    columns = dict(sums)
    columns.update(hullColumnsFromSums(sums, hullOffsets, hullPoints, hullReach, _segmentSums(a2, ro),
                                       _perId(_ringLengths(vo, v), ro, numpy.add, 0.0), missing))
    timings['columns'] = time.perf_counter() - t1
    timings['total'] = time.perf_counter() - t0
    return SegmentHulls(S, hullOffsets, hullPoints, hullReach, sums, columns, timings=timings, deviceMs=float(steps.sum()),
                        deviceStepsMs=dict(zip(HULL_STEPS, steps.tolist())), candidates=int(counts[1]), kept=int(counts[2]))


# ---- Douglas-Peucker simplification of the rings, shared borders staying shared (csrc/simplify.h) ------------------------
SIMPLIFY_STEPS = ('arcs', 'rounds', 'areas', 'emit')
SIMPLIFY_PATHS = {'auto': 0, 'short': 1, 'group': 2, 'global': 3}
MAX_TOLERANCE = 32768.0
# vertices one simplification can take (csrc/simplify.h: SP_MAX_VERTS)
MAX_SIMPLIFY_VERTICES = 2 ** 31 - 8192


def tolerance2q(tolerance):
    """T = floor(tolerance^2 * 65536), the integer the GPU compares with: a point at the cross product m from the chord
    of squared length l exceeds the tolerance when m^2 * 65536 > T * l.  ``tolerance`` is a float64 in vertex units,
    0 <= tolerance <= 32768 (T <= 2^46)."""
    try:
        t = float(tolerance)
    except (TypeError, ValueError):
        raise PyShepSegOutlinesError("tolerance must be a number 0 .. {} (got {!r})".format(int(MAX_TOLERANCE), tolerance))
    if isinstance(tolerance, (bool, numpy.bool_)) or not 0.0 <= t <= MAX_TOLERANCE:       # (a NaN fails both comparisons)
        raise PyShepSegOutlinesError("tolerance must be a number 0 .. {} (got {!r})".format(int(MAX_TOLERANCE), tolerance))
    return int(numpy.floor(t * t * 65536.0))


class SimplifiedOutlines(SegmentOutlines):
    """The result of simplifySegmentOutlines: a SegmentOutlines (so toWKT, writeGeoJSON, columnsFromRings and
    calcSegmentHulls take it) whose rings are the kept vertices of the rings of ``source``.

    ``sourceRing``: int64, the index of each surviving ring in ``source``; ``keptVertex``: int64, the index into
    ``source.vertices`` of every vertex; ``droppedRings``: int64, per id the rings of ``source`` that did not survive
    (also in ``columns``); ``junction``: the source's flags of the kept vertices; ``tolerance`` and ``tolerance2q``;
    ``rounds``: the depth of the recursion, the rounds in which an interval split; ``arcs``, ``longestArc``,
    ``arcClasses`` (arcs taken by the short, group and global kernels); ``timings``, ``deviceMs``, ``deviceStepsMs``
    (split into SIMPLIFY_STEPS) as its siblings have them."""
    def __init__(self, source, ringOffsets, vertexOffsets, vertices, ringArea2, sourceRing, keptVertex, tolerance=0.0,
                 tolerance2q=0, rounds=0, arcs=None, longestArc=None, arcClasses=None, timings=None, deviceMs=None,
                 deviceStepsMs=None):
        junction = None
        if getattr(source, 'junction', None) is not None:
            junction = numpy.ascontiguousarray(numpy.asarray(source.junction)[keptVertex])
        SegmentOutlines.__init__(self, source.maxSegId, ringOffsets, vertexOffsets, vertices, ringArea2, origin=source.origin,
                                 fourConnected=source.fourConnected, rounds=rounds, edges=source.edges, timings=timings,
                                 deviceMs=deviceMs, deviceStepsMs=deviceStepsMs, junction=junction)
        self.source = source
        self.sourceRing = sourceRing
        self.keptVertex = keptVertex
        self.tolerance = tolerance
        self.tolerance2q = tolerance2q
        self.arcs = arcs
        self.longestArc = longestArc
        self.arcClasses = arcClasses if arcClasses is not None else {}
        self.droppedRings = (numpy.diff(numpy.asarray(source.ringOffsets)) - numpy.diff(numpy.asarray(ringOffsets))).astype(numpy.int64)
        self.columns['droppedRings'] = self.droppedRings

    def _holeShells(self, segId):
        was = self.source._holeShells(segId)
        now = {int(self.sourceRing[r]): r for r in self._ringRange(segId)}
        owner = {}
        for (s, r) in now.items():
            if self.ringArea2[r] < 0 and was.get(s) in now and self.ringArea2[now[was[s]]] > 0:
                owner[r] = now[was[s]]
        return owner

    def polygonsOf(self, segId):
        """The id's polygons: a list of [shell, hole, ...], the shells in ring order.  A hole belongs to the shell its
        source ring belongs to in ``source.polygonsOf``, mapped through ``sourceRing`` (the ray test of the base class
        holds for rectilinear rings only); a hole whose shell was dropped is left out."""
        return SegmentOutlines.polygonsOf(self, segId)


def simplifySegmentOutlines(o, tolerance, path='auto'):
    """
    Topology-aware Douglas-Peucker simplification of all rings of a junction trace ``o`` on the GPU
    (csrc/simplify.h): a SimplifiedOutlines.  ``tolerance`` is in vertex units, 0 <= tolerance <= 32768.

    The rings are cut into arcs at their junction vertices (``o.junction``; a ring without any is one closed arc from
    its vertex of the smallest (row, col)), and every arc is simplified on its own with both ends kept: between kept
    points a and b the point of the largest distance from the chord a b is kept if that distance exceeds the
    tolerance, and both halves are treated the same way (module docstring for the exact integer rule).  An arc is run
    in opposite directions by the two rings that share it and every quantity is symmetric, so neighbours keep identical
    vertices along a shared border: no slivers, no overlaps.  Arcs may still cross each other at large tolerances;
    that is not checked.  A ring is dropped when fewer than three vertices remain or when its new ``ringArea2`` is 0 or
    differs in sign from its source ring's; the surviving rings keep their order.

    If ``o``'s rings are still the ones its trace left in HBM they are read in place; otherwise the rings and the
    flags are uploaded once, which also serves rings built by hand (``SegmentOutlines(..., junction=flags)``).
    ``path`` ('auto', 'short', 'group', 'global') forces one of the three arc size classes of the kernels for all arcs
    that fit it, so that tests and measurements reach each class at any size; the result does not depend on it.

    Refused before the GPU is touched: an ``o`` without ``junction`` (trace with ``junctions=True``), a tolerance
    that is negative, NaN or above 32768, flags that are not uint8 of the vertices' length, the coordinate spans
    calcSegmentHulls refuses, more than 2^31 - 8192 vertices, an unknown ``path``, and a working set larger than the
    free HBM.
    """
    t0 = time.perf_counter()
    if getattr(o, 'junction', None) is None:
        raise PyShepSegOutlinesError("these outlines carry no junction flags: trace them with junctions=True")
    T = tolerance2q(tolerance)
    (ro, vo, v, a2, base, span) = _checkRings(o)
    j = numpy.asarray(o.junction)
    if j.dtype != numpy.uint8 or j.ndim != 1 or len(j) != len(v):
        raise PyShepSegOutlinesError("junction must be a uint8 array with one entry per vertex ({})".format(len(v)))
    j = numpy.ascontiguousarray(j)
    if len(v) > MAX_SIMPLIFY_VERTICES or len(a2) > MAX_SIMPLIFY_VERTICES:
        raise PyShepSegOutlinesError("{} vertices in {} rings: more than the {} one simplification can take".format(
            len(v), len(a2), MAX_SIMPLIFY_VERTICES))
    if not isinstance(path, str) or path not in SIMPLIFY_PATHS:
        raise PyShepSegOutlinesError("path must be one of 'auto', 'short', 'group', 'global' (got {!r})".format(path))
    path = SIMPLIFY_PATHS[path]
    S = int(o.maxSegId)
    c = _lib.ctx()
    L = c._L
    timings = {}
    _takeRings(c, o, (ro, vo, v, a2, j), L.shp_simplify_need, L.shp_simplify_source, 'simplification', timings, t0)
    t1 = time.perf_counter()
    counts = numpy.zeros(10, dtype=numpy.int64)
    steps = numpy.zeros(4, dtype=numpy.float64)
    c.check(L.shp_simplify_build(c.handle, T, path, base[0], base[1], span[0], span[1], _lib.ptr(counts), _lib.ptr(steps)))
    timings['build'] = time.perf_counter() - t1
    t1 = time.perf_counter()
    (nr2, nv2) = (int(counts[0]), int(counts[1]))
    ringOffsets = numpy.empty(S + 2, dtype=numpy.int64)
    vertexOffsets = numpy.empty(nr2 + 1, dtype=numpy.int64)
    vertices = numpy.empty((nv2, 2), dtype=numpy.int64)
    ringArea2 = numpy.empty(nr2, dtype=numpy.int64)
    sourceRing = numpy.empty(nr2, dtype=numpy.int64)
    keptVertex = numpy.empty(nv2, dtype=numpy.int64)
    c.check(L.shp_simplify_download(c.handle, _lib.ptr(ringOffsets), _lib.ptr(vertexOffsets), _lib.ptr(vertices), _lib.ptr(ringArea2),
                                    _lib.ptr(sourceRing), _lib.ptr(keptVertex)))
    timings['download'] = time.perf_counter() - t1
    t1 = time.perf_counter()
    out = SimplifiedOutlines(o, ringOffsets, vertexOffsets, vertices, ringArea2, sourceRing, keptVertex, tolerance=float(tolerance),
                             tolerance2q=T, rounds=int(counts[2]), arcs=int(counts[3]), longestArc=int(counts[4]),
                             arcClasses={'short': int(counts[5]), 'group': int(counts[6]), 'global': int(counts[7])},
                             deviceMs=float(steps.sum()), deviceStepsMs=dict(zip(SIMPLIFY_STEPS, steps.tolist())))
    timings['columns'] = time.perf_counter() - t1
    timings['total'] = time.perf_counter() - t0
    out.timings = timings
    return out
