"""Drop-in for the colour-table part of ``pyshepseg.utils`` (utils.py:123-230), plus the rendering
that makes a colour table visible where the output is a ``.npy`` file.

``writeColorTableFromRatColumns(segfile, redColName, greenColName, blueColName)`` stretches three
columns (usually the per-segment means of three bands, e.g. out of
``tilingstats.calcPerSegmentStatsTiledBands``) between their 5th and 95th percentiles into the
byte columns Red, Green and Blue, and sets Alpha to 255.  The reference does this with two
``numpy.percentile`` calls and a float64 expression per column; here the column goes to the GPU,
the four order statistics the two percentiles need come out of a radix selection
(csrc/colour.h), and the stretch kernel produces numpy's bytes exactly.

``writeRandomColourTable(outBand, nRows, seed=None)`` is the reference's random table (host only).

``renderColourTable(segfile, colours, outfile=None)`` paints the label raster through a table:
pixel = (Red, Green, Blue, Alpha)[label], a ``(rows, cols, 4)`` uint8 raster.

There is no CPU fallback: without a GPU the first and the last fail as every entry point of this
package does.
"""
import collections.abc
import ctypes

import numpy

from . import _lib
from . import labelsource
from . import shepseg
from . import tilingstats

GFT_Integer = 0                                             # gdal.GFT_Integer
GFU_Red, GFU_Green, GFU_Blue, GFU_Alpha = 6, 7, 8, 9        # gdal.GFU_*, so callers need not import GDAL
COLOUR_NAMES = ('Red', 'Green', 'Blue', 'Alpha')
_COLTYPE = {numpy.dtype(numpy.float64): 0, numpy.dtype(numpy.float32): 1, numpy.dtype(numpy.int64): 2}


class PyShepSegUtilsError(Exception):
    pass


class ColourTableResult(object):
    """``columns``: {'Red', 'Green', 'Blue', 'Alpha'} -> uint8 array, one row per segment id.
    ``stretch``: the (lo, hi) = (5th, 95th percentile) of the red, green and blue source columns as
    float64 (None for a random table).  ``deviceMs``: the GPU time of the three columns (None for a
    random table)."""
    def __init__(self, columns, stretch=None, deviceMs=None):
        self.columns = columns
        self.stretch = stretch
        self.deviceMs = deviceMs


def _stretchColumn(c, col):
    """(bytes, (lo, hi), device ms) of one column: utils.py:216-221 on the GPU"""
    col = numpy.asarray(col)
    if col.ndim != 1 or col.size == 0:
        raise PyShepSegUtilsError("a column must be a non-empty 1-D array")
    if col.dtype.kind in 'iub':
        if col.dtype == numpy.uint64 and int(col.max()) >= 1 << 63:
            raise PyShepSegUtilsError("integer column holds a magnitude of 2^53 or more: not exact in float64")
        col = col.astype(numpy.int64, copy=False)       # (the statistics' Integer columns are int64 already)
    elif col.dtype.kind == 'f':
        if col.dtype not in _COLTYPE:
            col = col.astype(numpy.float64)
    else:
        raise PyShepSegUtilsError("a column of type %s cannot be stretched" % col.dtype)
    col = numpy.ascontiguousarray(col)
    out = numpy.empty(len(col), dtype=numpy.uint8)
    lohi = numpy.zeros(2, dtype=numpy.float64)
    ms = ctypes.c_double(0)
    c.check(c._L.shp_colour_stretch(c.handle, _lib.ptr(col), _COLTYPE[col.dtype], len(col), _lib.ptr(out),
                                    _lib.ptr(lohi), ctypes.byref(ms)))
    return (out, (numpy.float64(lohi[0]), numpy.float64(lohi[1])), ms.value)


def _openRat(segfile):
    try:
        from osgeo import gdal
    except ImportError:
        raise PyShepSegUtilsError("GDAL (osgeo) is not importable here: pass the columns (a mapping of column "
                                  "name to array, or a TiledStatsResult)")
    ds = segfile if isinstance(segfile, gdal.Dataset) else gdal.Open(segfile, gdal.GA_Update)
    return (ds, ds.GetRasterBand(1).GetDefaultRAT())


def writeColorTableFromRatColumns(segfile, redColName, greenColName, blueColName):
    """
    Use the values of three columns to make the colour columns Red, Green, Blue and Alpha, so that
    the segmentation displays like those bands of the image (reference utils.py:162-230).  Per column

        lo, hi = numpy.percentile(col, 5), numpy.percentile(col, 95)
        clr = (255 * ((col - lo) / (hi - lo)).clip(0, 1)).astype(numpy.uint8)

    in float64 (a RAT hands every column over as float64 or int64; float32 columns of this
    package's statistics are widened first, which is exact), byte for byte what numpy gives.  Alpha
    is 255 in every row, row 0 included, and row 0 takes part in the percentiles: both as in the
    reference.

    ``segfile`` is a mapping of column name to 1-D array (``TiledStatsResult.columns``), a
    ``TiledStatsResult``, or a GDAL file name / Dataset: then the columns are read from its RAT and
    the colour columns created there (Integer, usage GFU_Red / Green / Blue / Alpha) or reused by
    name, and written in the reference's order.  Returns a ColourTableResult.

    Where the reference's expression breaks down: ``hi == lo`` divides by zero there, and numpy on
    x86-64 ends with 255 where col > lo and 0 elsewhere (the NaN of col == lo casts to 0): exactly
    that is produced, without a NaN.  A NaN or an infinity in a column is an error (the reference
    turns the whole column into NaN), as is an integer of magnitude 2^53 or more (not exact in
    float64).  A column name that the table does not have is an error before anything is computed.
    """
    names = (redColName, greenColName, blueColName)
    (ds, attrTbl) = (None, None)
    if isinstance(segfile, tilingstats.TiledStatsResult):
        if segfile.columns is None:
            raise PyShepSegUtilsError("the statistics' columns went to the segment file: pass that file")
        table = segfile.columns
    elif isinstance(segfile, collections.abc.Mapping):
        table = segfile
    else:
        (ds, attrTbl) = _openRat(segfile)
        colNameList = [attrTbl.GetNameOfCol(i) for i in range(attrTbl.GetColumnCount())]
        table = colNameList
    for n in names:
        if n not in table:
            raise PyShepSegUtilsError("column '{}' is not in the table".format(n))
    if ds is None:
        if len(set(len(table[n]) for n in names)) != 1:
            raise PyShepSegUtilsError("the three columns differ in length")
    c = _lib.ctx()
    columns = {}
    stretch = []
    deviceMs = 0.0

    def store(colourName, usage, values):
        if colourName not in colNameList:
            attrTbl.CreateColumn(colourName, GFT_Integer, usage)
            colNameList.append(colourName)
        attrTbl.WriteArray(values, colNameList.index(colourName))

    for (n, colourName, usage) in zip(names, COLOUR_NAMES, (GFU_Red, GFU_Green, GFU_Blue)):
        colVals = table[n] if ds is None else attrTbl.ReadAsArray(colNameList.index(n))
        (clr, lohi, ms) = _stretchColumn(c, colVals)
        columns[colourName] = clr
        stretch.append(lohi)
        deviceMs += ms
        if ds is not None:
            store(colourName, usage, clr)
    columns['Alpha'] = numpy.full(len(columns['Red']), 255, dtype=numpy.uint8)
    if ds is not None:
        store('Alpha', GFU_Alpha, columns['Alpha'])
        ds.FlushCache()
    return ColourTableResult(columns, stretch, deviceMs)


def writeRandomColourTable(outBand, nRows, seed=None):
    """
    A random colour table of nRows rows (the number of segments + 1), useful to see the segment
    boundaries (reference utils.py:123-159): Red, Green and Blue uniform in 0..255, Alpha 255 and 0
    for the null segment's row.  ``outBand`` is a GDAL band -- its RAT gets nRows rows and the four
    columns, found by their usage or created Integer in the reference's order (Blue, Green, Red,
    Alpha) -- or None to only return the ColourTableResult.  The reference draws from numpy's
    unseeded global generator; here ``numpy.random.default_rng(seed)``.
    """
    nRows = int(nRows)
    if nRows < 1:
        raise PyShepSegUtilsError("nRows must be at least 1 (the null segment's row)")
    rng = numpy.random.default_rng(seed)
    columns = {}
    attrTbl = None
    if outBand is not None:
        attrTbl = outBand.GetDefaultRAT()
        attrTbl.SetRowCount(nRows)

    def store(name, usage, values):
        if attrTbl is None:
            return
        colNum = attrTbl.GetColOfUsage(usage)
        if colNum == -1:
            attrTbl.CreateColumn(name, GFT_Integer, usage)
            colNum = attrTbl.GetColumnCount() - 1
        attrTbl.WriteArray(values, colNum)

    for (name, usage) in (('Blue', GFU_Blue), ('Green', GFU_Green), ('Red', GFU_Red)):
        columns[name] = rng.integers(0, 256, size=nRows, dtype=numpy.uint8)
        store(name, usage, columns[name])
    columns['Alpha'] = numpy.full(nRows, 255, dtype=numpy.uint8)
    columns['Alpha'][shepseg.SEGNULLVAL] = 0
    store('Alpha', GFU_Alpha, columns['Alpha'])
    return ColourTableResult(columns)


def _colourColumns(colours):
    """the four columns of `colours` as uint8 arrays of one length"""
    table = colours.columns if isinstance(colours, ColourTableResult) else colours
    if not isinstance(table, collections.abc.Mapping):
        raise PyShepSegUtilsError("colours must be a ColourTableResult or a mapping with the columns %s"
                                  % ', '.join(COLOUR_NAMES))
    cols = []
    for name in COLOUR_NAMES:
        if name not in table:
            raise PyShepSegUtilsError("colours has no column '{}'".format(name))
        col = numpy.asarray(table[name])
        if col.ndim != 1 or col.dtype.kind not in 'iu':
            raise PyShepSegUtilsError("colour column '{}' must be a 1-D integer array".format(name))
        if len(col) != len(numpy.asarray(table[COLOUR_NAMES[0]])):
            raise PyShepSegUtilsError("colour column '{}' has {} rows, '{}' has {}".format(
                name, len(col), COLOUR_NAMES[0], len(numpy.asarray(table[COLOUR_NAMES[0]]))))
        if col.dtype != numpy.uint8:
            if len(col) and (col.min() < 0 or col.max() > 255):
                raise PyShepSegUtilsError("colour column '{}' holds values outside 0..255".format(name))
            col = col.astype(numpy.uint8)
        cols.append(numpy.ascontiguousarray(col))
    if len(cols[0]) == 0:
        raise PyShepSegUtilsError("the colour table is empty")
    return cols


def renderColourTable(segfile, colours, outfile=None, chunkPixels=None):
    """
    The label raster painted through a colour table: the (rows, cols, 4) uint8 raster whose pixel
    is (Red, Green, Blue, Alpha)[label].  ``segfile`` is a 2-D uint32 array, a ``.npy`` path, or
    the result of ``doTiledShepherdSegmentation(..., outfile=tiling._KEEP_ON_DEVICE)`` whose labels
    are in HBM; ``colours`` the result of writeColorTableFromRatColumns / writeRandomColourTable, or
    a mapping with the columns Red, Green, Blue and Alpha.  With ``outfile`` (a ``.npy`` path) the
    raster is written there and None returned, else the array is returned.

    The labels stream through the GPU in row blocks of ``chunkPixels`` pixels (default
    tilingstats.STATS_CHUNK_PIXELS), as the statistics stream them, so the raster may be larger than
    HBM and than a 32-bit pixel index.  A label that has no row in the table is an error that names it.
    """
    cols = _colourColumns(colours)
    nTable = len(cols[0])
    if outfile is not None and not (isinstance(outfile, str) and outfile.endswith('.npy')):
        raise PyShepSegUtilsError("outfile must be None or a .npy path")
    labels = labelsource.resolve(segfile, None, PyShepSegUtilsError)
    c = _lib.ctx()
    L = c._L
    dTable = ctypes.c_void_p()

    def lookup(y0, y1, dseg, dout):
        c.check(L.shp_colour_lookup_dev(c.handle, dseg, (y1 - y0) * labels.ncols, dTable, nTable, dout))
        return True

    try:
        with labelsource.LabelSource(c, labels) as src:
            c.check(L.shp_dev_alloc(c.handle, nTable * 4, ctypes.byref(dTable)))
            c.check(L.shp_colour_pack(c.handle, _lib.ptr(cols[0]), _lib.ptr(cols[1]), _lib.ptr(cols[2]), _lib.ptr(cols[3]),
                                      nTable, dTable))
            return labelsource.mapBlocks(src, chunkPixels, lookup, numpy.uint8, pixelShape=(4,), outfile=outfile)
    finally:
        if dTable.value:
            c.check(L.shp_dev_free(c.handle, dTable))
