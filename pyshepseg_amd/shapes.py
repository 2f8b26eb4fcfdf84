"""Per-segment shape attributes of a label raster: extent, centroid, perimeter, compactness, elongation, orientation.

An object-based workflow classifies segments on what they look like (tilingstats.calcPerSegmentStatsTiledBands), on
what lies around them (neighbours.findSegmentNeighbours, reduceOverNeighbours) and on what shape they have.
``calcSegmentShapes`` answers the third from the label raster alone, on the GPU (csrc/segshape.h): one pass over the
labels in row blocks gives, per segment id, integer counts and coordinate sums, and ``shapeColumnsFromSums`` derives
the float columns from those on the host.

Definitions, with (r, c) a pixel's coordinates counted from ``origin`` and label 0 no segment:

``area``: pixels of the id.  ``rowMin``, ``rowMax``, ``colMin``, ``colMax``: its extent.  ``perimeter``: the sides
(N, S, W, E) of the id's pixels whose other side is a different label, label 0 or outside the raster;
``outerBorder``: those of them whose other side is label 0 or outside the raster; ``edgePixels``: pixels of the id with
at least one such side.  So ``perimeter == findSegmentNeighbours(seg, fourConnected=True).columns['borderLength'] +
outerBorder``, and ``nb.columns['borderLength'] / perimeter`` is the segment's relative border to other segments.
``sums``: the sums of r, c, r^2, c^2 and r c over the id's pixels modulo 2^64 (numpy's wrap).

There is no CPU fallback: without a GPU the call fails as every entry point of this package does.  The multi-rank
form on row-sharded labels is dist_shapes.calcSegmentShapesDistributed (distributed.calcSegmentShapesDistributed): every
rank accumulates its rows with its first row as the row origin and a halo row on either side, only the segments that
straddle a cut travel, and the result is this function's on the whole mosaic, bit for bit.
"""
import ctypes
import time

import numpy

from . import _lib
from . import labelsource


class PyShepSegShapesError(Exception):
    pass


COUNT_COLUMNS = ('area', 'rowMin', 'rowMax', 'colMin', 'colMax', 'perimeter', 'outerBorder', 'edgePixels')
SUM_COLUMNS = ('sumRow', 'sumCol', 'sumRowRow', 'sumColCol', 'sumRowCol')
DERIVED_COLUMNS = ('centroidRow', 'centroidCol', 'bboxFill', 'compactness', 'elongation', 'orientation')
# words of an id's row of the device table (csrc/segshape.h)
_TABLE_WORDS = 11
_SUM_WORD = {'sumRow': 1, 'sumCol': 2, 'sumRowRow': 3, 'sumColCol': 4, 'sumRowCol': 5}
_COUNT_WORD = {'area': 0, 'perimeter': 6, 'outerBorder': 7, 'edgePixels': 8}


class SegmentShapes(object):
    """The result of calcSegmentShapes.  Every array has ``maxSegId + 1`` rows; row 0 and ids without pixels hold 0
    in integer columns and ``missingStatsValue`` in float columns.

    ``columns``: the int64 columns COUNT_COLUMNS and the float64 columns DERIVED_COLUMNS, as the statistics' column
    dictionaries hold them; ``sums``: the uint64 columns SUM_COLUMNS; ``origin``: (row0, col0), the coordinates of the
    raster's first pixel; ``timings``: seconds per step; ``deviceMs``: GPU time of the kernels."""
    def __init__(self, maxSegId, columns, sums, origin, timings=None, deviceMs=None):
        self.maxSegId = maxSegId
        self.columns = columns
        self.sums = sums
        self.origin = origin
        self.timings = timings if timings is not None else {}
        self.deviceMs = deviceMs


def shapeColumnsFromSums(counts, sums, missingStatsValue=-9999):
    """
    The float64 columns DERIVED_COLUMNS from the counted columns (``counts``: int64 'area', 'rowMin', 'rowMax',
    'colMin', 'colMax', 'perimeter') and the moment sums (``sums``: uint64 SUM_COLUMNS, modulo 2^64), as a dictionary.

    The sums are first shifted to the bounding box in uint64 arithmetic (m1r = sumRow - area rowMin, m2rr = sumRowRow -
    2 rowMin sumRow + area rowMin^2, m2rc = sumRowCol - rowMin sumCol - colMin sumRow + area rowMin colMin, and the
    same for columns): the wrap cancels, and the shifted values are exact whenever area * max(h - 1, w - 1)^2 < 2^64,
    wherever the segment lies.  With a = area, mr = m1r / a, mc = m1c / a: vrr = m2rr / a - mr^2 + 1/12, vcc likewise,
    vrc = m2rc / a - mr mc (1/12: a pixel's own extent); lmax, lmin = (vrr + vcc +- sqrt((vrr - vcc)^2 + 4 vrc^2)) / 2.

    ``centroidRow``, ``centroidCol``: rowMin + mr, colMin + mc; ``bboxFill``: area / (h w); ``compactness``:
    4 pi area / perimeter^2; ``elongation``: sqrt(lmax / lmin) >= 1; ``orientation``: 0.5 arctan2(2 vrc, vcc - vrr),
    the angle of the major axis from the column axis towards increasing row, in radians.  Rows with area 0 hold
    ``missingStatsValue``.
    """
    u64 = numpy.uint64
    area = numpy.asarray(counts['area'])
    out = {name: numpy.full(len(area), float(missingStatsValue), dtype=numpy.float64) for name in DERIVED_COLUMNS}
    rows = numpy.flatnonzero(area > 0)
    if len(rows) == 0:
        return out
    n = area[rows].astype(u64)
    (rmin, rmax) = (numpy.asarray(counts['rowMin'])[rows].astype(u64), numpy.asarray(counts['rowMax'])[rows].astype(u64))
    (cmin, cmax) = (numpy.asarray(counts['colMin'])[rows].astype(u64), numpy.asarray(counts['colMax'])[rows].astype(u64))
    (sr, sc, srr, scc, src) = (numpy.asarray(sums[name])[rows].astype(u64) for name in SUM_COLUMNS)
    two = u64(2)
    # modulo 2^64 throughout: numpy's integer arrays wrap
    m1r = sr - n * rmin
    m1c = sc - n * cmin
    m2rr = srr - two * rmin * sr + n * rmin * rmin
    m2cc = scc - two * cmin * sc + n * cmin * cmin
    m2rc = src - rmin * sc - cmin * sr + n * rmin * cmin
    a = n.astype(numpy.float64)
    mr = m1r.astype(numpy.float64) / a
    mc = m1c.astype(numpy.float64) / a
    vrr = m2rr.astype(numpy.float64) / a - mr * mr + 1.0 / 12.0
    vcc = m2cc.astype(numpy.float64) / a - mc * mc + 1.0 / 12.0
    vrc = m2rc.astype(numpy.float64) / a - mr * mc
    t = vrr + vcc
    d = numpy.sqrt((vrr - vcc) ** 2 + 4.0 * vrc * vrc)
    lmax = (t + d) / 2.0
    lmin = (t - d) / 2.0
    h = (rmax - rmin + u64(1)).astype(numpy.float64)
    w = (cmax - cmin + u64(1)).astype(numpy.float64)
    perimeter = numpy.asarray(counts['perimeter'])[rows].astype(numpy.float64)
    out['centroidRow'][rows] = rmin.astype(numpy.float64) + mr
    out['centroidCol'][rows] = cmin.astype(numpy.float64) + mc
    out['bboxFill'][rows] = a / (h * w)
    out['compactness'][rows] = 4.0 * numpy.pi * a / (perimeter * perimeter)
    out['elongation'][rows] = numpy.sqrt(lmax / lmin)
    out['orientation'][rows] = 0.5 * numpy.arctan2(2.0 * vrc, vcc - vrr)
    return out


def _checkArgs(segfile, maxSegId, origin, chunkPixels, missingStatsValue):
    """(the labelsource.Labels of the raster, (row0, col0), chunkPixels, missing): everything that can be refused before
    the GPU is touched"""
    Err = PyShepSegShapesError
    labels = labelsource.resolve(segfile, maxSegId, Err, merged=True, hint=True)
    missing = labelsource.number(missingStatsValue, 'missingStatsValue', Err)
    origin = labelsource.checkOrigin(origin, labels.nrows, labels.ncols, Err)
    return (labels, origin, labelsource.checkChunkPixels(chunkPixels, Err), missing)


def calcSegmentShapes(segfile, maxSegId=None, origin=(0, 0), chunkPixels=None, missingStatsValue=-9999):
    """
    Shape attributes of every segment of a label raster, on the GPU: a SegmentShapes.

    ``segfile`` is what findSegmentNeighbours takes -- a 2-D uint32 array, a ``.npy`` path (memory-mapped: the raster
    may be larger than HBM), a TiledSegmentationResult (its ``segimg``), a result whose labels are in HBM (``outDev``,
    read in place) -- or a MergedSegments: its ``outDev`` if it has one, else its ``segimg``.

    ``maxSegId`` is the last row of every column.  None takes the ``maxSegId`` of a result object that carries one,
    otherwise the largest label, found by a reduction over the labels on the GPU before the accumulation: for a host
    array or a ``.npy`` path that is a second read (and upload) of the raster, which a given ``maxSegId`` saves.  A
    label above a given ``maxSegId`` raises PyShepSegShapesError with the largest such label.

    ``origin`` = (row0, col0), non-negative integers: pixel (y, x) of the raster has the coordinates (row0 + y,
    col0 + x) in every output (the raster as a window of a larger one).  Coordinates stay below 2^32.

    The labels stream through the GPU in row blocks of ``chunkPixels`` pixels (default tilingstats.STATS_CHUNK_PIXELS),
    each with the row above and below it; the result does not depend on the blocks.
    """
    (labels, origin, chunkPixels, missing) = _checkArgs(segfile, maxSegId, origin, chunkPixels, missingStatsValue)
    maxSegId = labels.maxSegId
    t0 = time.perf_counter()
    c = _lib.ctx()
    L = c._L
    timings = {}
    deviceMs = 0.0
    ms = ctypes.c_double(0)
    with labelsource.LabelSource(c, labels) as src:
        if maxSegId is None:
            (maxSegId, deviceMs) = src.labelMax(PyShepSegShapesError, chunkPixels)
            timings['labelMax'] = time.perf_counter() - t0
        t1 = time.perf_counter()
        c.check(L.shp_shape_begin(c.handle, maxSegId, origin[0], origin[1]))
        for (y0, y1, dseg, above, below) in src.blocks(chunkPixels, above=True, below=True):
            c.check(L.shp_shape_accumulate_dev(c.handle, dseg, y1 - y0, labels.ncols, int(above), int(below)))
        timings['accumulate'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        (S, bad) = (ctypes.c_uint32(0), ctypes.c_uint32(0))
        c.check(L.shp_shape_finish(c.handle, ctypes.byref(S), ctypes.byref(bad), ctypes.byref(ms)))
        deviceMs += ms.value
        if bad.value:
            raise PyShepSegShapesError("segment id {} is above maxSegId {}".format(bad.value, S.value))
        timings['finish'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        table = numpy.empty((S.value + 1, _TABLE_WORDS), dtype=numpy.uint64)
        c.check(L.shp_shape_download(c.handle, _lib.ptr(table)))
        timings['download'] = time.perf_counter() - t1
    t1 = time.perf_counter()
    (columns, sums) = columnsFromTable(table, missing)
    timings['derive'] = time.perf_counter() - t1
    timings['total'] = time.perf_counter() - t0
    return SegmentShapes(S.value, columns, sums, origin, timings=timings, deviceMs=deviceMs)


def columnsFromTable(table, missingStatsValue=-9999):
    """(columns, sums) of a SegmentShapes from the downloaded device table (maxSegId + 1 rows of _TABLE_WORDS uint64,
    csrc/segshape.h): what calcSegmentShapes and dist_shapes.deviceShapes both end with"""
    columns = {name: table[:, w].astype(numpy.int64) for (name, w) in _COUNT_WORD.items()}
    lo = numpy.uint64(0xFFFFFFFF)
    sh = numpy.uint64(32)
    columns['rowMin'] = (table[:, 9] & lo).astype(numpy.int64)
    columns['rowMax'] = (table[:, 9] >> sh).astype(numpy.int64)
    columns['colMin'] = (table[:, 10] & lo).astype(numpy.int64)
    columns['colMax'] = (table[:, 10] >> sh).astype(numpy.int64)
    sums = {name: numpy.ascontiguousarray(table[:, w]) for (name, w) in _SUM_WORD.items()}
    columns = {name: columns[name] for name in COUNT_COLUMNS}
    columns.update(shapeColumnsFromSums(columns, sums, missingStatsValue))
    return columns, sums
