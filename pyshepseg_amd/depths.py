"""Per-segment depth: the exact Euclidean distance transform of a label raster, the deepest pixel of every segment,
its core areas.

The other per-segment columns look at a segment from outside: its spectra (tilingstats), its neighbours (neighbours),
its shape sums (shapes), its outline (outlines).  ``calcSegmentDepths`` measures it from the inside, from the label
raster alone, on the GPU (csrc/segdepth.h): a point that is surely inside the segment (a label or seed point, where the
centroid of an L-shaped, ring-shaped or many-part segment lies outside it), how wide the segment is, and how many of
its pixels lie farther than an edge depth from its border (the landscape metrics' core area, and the mask to sample
training pixels from).

Definitions.  Label 0 is no segment.  A position q is foreign to a pixel p of label L != 0 when q lies outside the
raster or ``label(q) != L``: another id and label 0 alike, as ``perimeter`` counts sides.  ``depth2(p)`` is the minimum
over the foreign q of (py - qy)^2 + (px - qx)^2, and 0 where the label is 0.  So ``depth2 >= 1`` on every labelled pixel,
and ``depth2 == 1`` exactly on the pixels shapes.calcSegmentShapes counts as ``edgePixels``.  Distance is by label, not by
connectivity: one label in two parts is one label.  A call takes at most ``outlines.MAX_ITEMS`` pixels, so a depth is at
most 32768 and ``depth2 <= 2^30``.

Per id, in ``maxSegId + 1`` rows, int64: ``maxDepth2`` the largest depth2 of the id's pixels; ``interiorRow``,
``interiorCol`` the pixel that has it, ``origin`` added, of several the first in row-major order; ``sumDepth2`` the sum
of depth2 over the id's pixels; and per pair (name, depth) of ``coreAreas`` the count of the id's pixels with ``depth2 >
floor(depth^2)`` (depth 0: the area; depth 1: area - edgePixels).  float64, derived on the host: ``maxDepth`` =
sqrt(maxDepth2), ``meanDepth2`` = sumDepth2 / area, ``depthRatio`` = pi maxDepth2 / area, the share of the segment that
a disc of that radius would cover: near 1 for a disc, small for thin or ragged segments.

``maxDepth`` is a distance between pixel centres: from the centre of the interior pixel to the nearest pixel centre
that is not the segment's (or the nearest position outside the raster).  It is not the radius of a circle inscribed in
the pixel squares.

The labels are whole in HBM for this function: a host array or ``.npy`` file is uploaded once, resident labels are
read in place.  The working set is 4 bytes a pixel for labels that have to go up, 6 bytes a pixel for the column
distances (2) and depth2 (4), 20 bytes per column and band of 32 rows (0.625 a pixel), 12 bytes per 64 columns of a row
(0.19 a pixel), 88 bytes an id, 16 bytes per 65 pixels for the list of runs the envelope solves (16 a pixel with ``path='envelope'``), and 8 bytes per pixel of those
runs, known once the window has run; when the free HBM does not hold it the call raises before anything is allocated
(the table of a ``maxSegId`` that has to be found first, and the envelope's scratch, before they are).
There is no CPU fallback.  Streaming in row blocks and a multi-rank form do not exist yet.
"""
import ctypes
import time

import numpy

from . import _lib
from . import labelsource
from . import outlines


class PyShepSegDepthsError(Exception):
    pass


COUNT_COLUMNS = ('maxDepth2', 'interiorRow', 'interiorCol', 'sumDepth2')
DERIVED_COLUMNS = ('maxDepth', 'meanDepth2', 'depthRatio')
MAX_CORE_AREAS = 8
MAX_DEPTH = 32768.0
PATHS = ('auto', 'envelope')
STEPS = ('columns', 'window', 'envelope', 'reduce')
# words of an id's row of the device table (csrc/segdepth.h)
_TABLE_WORDS = 11
_CORE_WORD = 3


class SegmentDepths(object):
    """The result of calcSegmentDepths.  Every column has ``maxSegId + 1`` rows; row 0 and ids without pixels hold 0
    in integer columns and ``missingStatsValue`` in float columns.

    ``columns``: the int64 columns COUNT_COLUMNS and one per core area, and the float64 columns DERIVED_COLUMNS, as the
    statistics' column dictionaries hold them; ``origin``: (row0, col0); ``coreAreas``: the pairs (name, Q), a pixel
    counting for ``name`` when depth2 > Q; ``depth2``: the (nrows, ncols) uint32 raster with ``depthRaster=True``, else
    None; ``deferredPixels``: the pixels the window of the row step could not decide and the envelope solved (with
    ``path='envelope'``: the pixels of all runs the envelope solved, which is every labelled pixel); ``timings``:
    seconds per step; ``deviceMs``: GPU time of the kernels, ``deviceStepsMs`` its split into STEPS."""
    def __init__(self, maxSegId, columns, origin, coreAreas, depth2=None, deferredPixels=0, timings=None, deviceMs=None,
                 deviceStepsMs=None):
        self.maxSegId = maxSegId
        self.columns = columns
        self.origin = origin
        self.coreAreas = coreAreas
        self.depth2 = depth2
        self.deferredPixels = deferredPixels
        self.timings = timings if timings is not None else {}
        self.deviceMs = deviceMs
        self.deviceStepsMs = deviceStepsMs if deviceStepsMs is not None else {}


def depth2q(depth):
    """Q = floor(depth^2), the integer the GPU compares with: a pixel lies in the core when depth2 > Q.  ``depth`` is a
    float64, 0 <= depth <= 32768 (Q <= 2^30)."""
    try:
        d = float(depth)
    except (TypeError, ValueError):
        raise PyShepSegDepthsError("an edge depth must be a number 0 .. {} (got {!r})".format(int(MAX_DEPTH), depth))
    if isinstance(depth, (bool, numpy.bool_)) or not 0.0 <= d <= MAX_DEPTH:          # (a NaN fails both comparisons)
        raise PyShepSegDepthsError("an edge depth must be a number 0 .. {} (got {!r})".format(int(MAX_DEPTH), depth))
    return int(numpy.floor(d * d))


def checkCoreAreas(coreAreas):
    """the pairs (name, Q) of ``coreAreas``, a sequence of at most MAX_CORE_AREAS pairs (columnName, depth)"""
    try:
        pairs = [tuple(p) for p in coreAreas]
    except TypeError:
        raise PyShepSegDepthsError("coreAreas must be a sequence of (columnName, depth) pairs (got {!r})".format(coreAreas))
    if len(pairs) > MAX_CORE_AREAS:
        raise PyShepSegDepthsError("{} core areas: at most {} in one call".format(len(pairs), MAX_CORE_AREAS))
    out = []
    for p in pairs:
        if len(p) != 2 or not isinstance(p[0], str):
            raise PyShepSegDepthsError("coreAreas must be a sequence of (columnName, depth) pairs (got {!r})".format(p))
        (name, depth) = p
        if name in COUNT_COLUMNS or name in DERIVED_COLUMNS:
            raise PyShepSegDepthsError("core area {!r} has the name of a fixed column".format(name))
        if name in [n for (n, _q) in out]:
            raise PyShepSegDepthsError("core area {!r} is named twice".format(name))
        out.append((name, depth2q(depth)))
    return out


def _checkArgs(segfile, maxSegId, origin, coreAreas, path, missingStatsValue):
    """(the labelsource.Labels of the raster, (row0, col0), the core areas' pairs (name, Q), missing): everything that can
    be refused before the GPU is touched; the raster, ``maxSegId``, ``missingStatsValue`` and ``origin`` as
    shapes.calcSegmentShapes takes them"""
    Err = PyShepSegDepthsError
    cores = checkCoreAreas(coreAreas)
    if path not in PATHS:
        raise Err("path must be one of {} (got {!r})".format(PATHS, path))
    labels = labelsource.resolve(segfile, maxSegId, Err, merged=True, hint=True)
    missing = labelsource.number(missingStatsValue, 'missingStatsValue', Err)
    origin = labelsource.checkOrigin(origin, labels.nrows, labels.ncols, Err)
    if labels.nrows * labels.ncols > outlines.MAX_ITEMS:
        raise Err("a raster of {} pixels: more than the {} one call can take".format(labels.nrows * labels.ncols,
                                                                                     outlines.MAX_ITEMS))
    return (labels, origin, cores, missing)


def depthColumnsFromTable(table, ncols, origin, cores, missingStatsValue=-9999):
    """The columns of a SegmentDepths from the downloaded device table (maxSegId + 1 rows of _TABLE_WORDS uint64,
    csrc/segdepth.h: pixels, sum of depth2, depth2 << 32 | 0xFFFFFFFF - linear index of the deepest pixel, a count per
    core area) of a raster ``ncols`` wide; ``cores`` the pairs (name, Q)."""
    area = table[:, 0].astype(numpy.int64)
    has = area > 0
    key = table[:, 2]
    linear = (numpy.uint64(0xFFFFFFFF) - (key & numpy.uint64(0xFFFFFFFF))).astype(numpy.int64)
    columns = {}
    columns['maxDepth2'] = (key >> numpy.uint64(32)).astype(numpy.int64)
    columns['interiorRow'] = numpy.where(has, origin[0] + linear // max(ncols, 1), 0).astype(numpy.int64)
    columns['interiorCol'] = numpy.where(has, origin[1] + linear % max(ncols, 1), 0).astype(numpy.int64)
    columns['sumDepth2'] = table[:, 1].astype(numpy.int64)
    for (k, (name, _q)) in enumerate(cores):
        columns[name] = table[:, _CORE_WORD + k].astype(numpy.int64)
    derived = {name: numpy.full(len(area), float(missingStatsValue), dtype=numpy.float64) for name in DERIVED_COLUMNS}
    a = area[has].astype(numpy.float64)
    m2 = columns['maxDepth2'][has].astype(numpy.float64)
    derived['maxDepth'][has] = numpy.sqrt(m2)
    derived['meanDepth2'][has] = columns['sumDepth2'][has].astype(numpy.float64) / a
    derived['depthRatio'][has] = numpy.pi * m2 / a
    columns.update(derived)
    return columns


def calcSegmentDepths(segfile, maxSegId=None, origin=(0, 0), coreAreas=(), depthRaster=False, path='auto',
                      missingStatsValue=-9999):
    """
    How deep every segment of a label raster is, on the GPU: a SegmentDepths (module docstring for the definitions).

    ``segfile`` is what outlines.traceSegmentOutlines takes -- a 2-D uint32 array, a ``.npy`` path, a
    TiledSegmentationResult (its ``segimg``), a result whose labels are in HBM (``outDev``, read in place) or a
    MergedSegments (its ``outDev`` if it has one, else its ``segimg``).  A host raster is uploaded once, whole.

    ``maxSegId`` is the last row of every column; None takes the ``maxSegId`` of a result object that carries one,
    otherwise the largest label, found by a reduction on the GPU.  A label above a given ``maxSegId`` raises
    PyShepSegDepthsError with the largest such label.  ``origin`` = (row0, col0), non-negative integers, is added to
    ``interiorRow`` and ``interiorCol`` and changes nothing else.

    ``coreAreas``: at most 8 pairs (columnName, depth), depth a number 0 .. 32768; each gives an int64 column of that
    name, the id's pixels farther than ``depth`` from its border: depth2 > floor(depth^2).

    ``depthRaster=True`` downloads the per-pixel result into ``depth2``; otherwise it never leaves the device.

    ``path``: 'auto' decides every pixel it can in a window of the row and solves only the row runs that hold an
    undecided pixel by their lower envelope; 'envelope' solves every run that way.  The result does not depend on it.

    The raster has at most 2^32 - 8192 pixels, and the working set (module docstring) must fit the free HBM: otherwise
    PyShepSegDepthsError names the bytes needed, before anything is allocated.
    """
    (labels, origin, cores, missing) = _checkArgs(segfile, maxSegId, origin, coreAreas, path, missingStatsValue)
    (nrows, ncols, maxSegId) = (labels.nrows, labels.ncols, labels.maxSegId)
    allRuns = int(path == 'envelope')
    t0 = time.perf_counter()
    c = _lib.ctx()
    L = c._L
    npix = nrows * ncols
    timings = {}
    (need, free) = (ctypes.c_int64(0), ctypes.c_int64(0))
    deviceMs = 0.0
    with labelsource.LabelSource(c, labels) as src:
        # (the table of a maxSegId that is not known yet is checked once it is: below)
        c.check(L.shp_depth_need(c.handle, nrows, ncols, maxSegId if maxSegId is not None else 0, allRuns, -1,
                                 ctypes.byref(need), ctypes.byref(free)))
        want = need.value + (4 * npix if labels.devSeg is None else 0)
        if want > free.value:
            raise PyShepSegDepthsError("the labels, per-pixel arrays and per-id table of {} x {} pixels need {} bytes of device "
                                       "memory, {} are free".format(nrows, ncols, want, free.value))
        dseg = src.whole()
        timings['upload'] = time.perf_counter() - t0
        if maxSegId is None:
            t1 = time.perf_counter()
            (maxSegId, deviceMs) = src.labelMax(PyShepSegDepthsError)
            c.check(L.shp_depth_need(c.handle, nrows, ncols, maxSegId, allRuns, -1, ctypes.byref(need), ctypes.byref(free)))
            if need.value > free.value:
                raise PyShepSegDepthsError("the per-pixel arrays and the per-id table of {} ids need {} bytes of device memory, "
                                           "{} are free".format(maxSegId + 1, need.value, free.value))
            timings['labelMax'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        counts = numpy.zeros(3, dtype=numpy.int64)
        c.check(L.shp_depth_transform_dev(c.handle, dseg, nrows, ncols, allRuns, _lib.ptr(counts)))
        (deferred, _nruns, room) = (int(v) for v in counts)
        timings['transform'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        if room:
            c.check(L.shp_depth_need(c.handle, nrows, ncols, maxSegId, allRuns, room, ctypes.byref(need), ctypes.byref(free)))
            if need.value > free.value:
                raise PyShepSegDepthsError("the envelope's scratch of {} positions needs {} bytes of device memory, {} are "
                                           "free".format(room, need.value, free.value))
        c.check(L.shp_depth_envelope(c.handle))
        timings['envelope'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        q = numpy.array([v for (_n, v) in cores] + [0] * (MAX_CORE_AREAS - len(cores)), dtype=numpy.uint32)
        steps = numpy.zeros(4, dtype=numpy.float64)
        bad = ctypes.c_uint32(0)
        c.check(L.shp_depth_reduce(c.handle, maxSegId, len(cores), _lib.ptr(q), ctypes.byref(bad), _lib.ptr(steps)))
        if bad.value:
            raise PyShepSegDepthsError("segment id {} is above maxSegId {}".format(bad.value, maxSegId))
        timings['reduce'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        table = numpy.empty((maxSegId + 1, _TABLE_WORDS), dtype=numpy.uint64)
        depth2 = numpy.empty((nrows, ncols), dtype=numpy.uint32) if depthRaster else None
        c.check(L.shp_depth_download(c.handle, _lib.ptr(table), _lib.ptr(depth2) if depthRaster and npix else None))
        timings['download'] = time.perf_counter() - t1
    deviceStepsMs = dict(zip(STEPS, steps.tolist()))
    deviceMs += float(steps.sum())
    t1 = time.perf_counter()
    columns = depthColumnsFromTable(table, ncols, origin, cores, missing)
    timings['derive'] = time.perf_counter() - t1
    timings['total'] = time.perf_counter() - t0
    if allRuns:
        deferred = int(table[:, 0].sum())
    return SegmentDepths(maxSegId, columns, origin, cores, depth2=depth2, deferredPixels=deferred, timings=timings,
                         deviceMs=deviceMs, deviceStepsMs=deviceStepsMs)
