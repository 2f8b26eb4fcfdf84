"""
Subset a segmentation so that only the segments present in the subset remain, renumbered in
first-seen order -- the compute step of the reference's ``pyshepseg.subset.subsetImage``
(subset.py:39-227) on the GPU (``shp_subset_recode``).

Rasters are numpy arrays / ``.npy`` paths (GDAL is optional and absent on the build machines);
the RAT of the reference becomes a dict of column arrays (``ratColumns``), every column row-
gathered to the new ids exactly as ``copySubsettedSegmentsToNew`` (subset.py:232-266) does.
"""
import ctypes

import numpy

from . import _lib
from . import shepseg
from . import tiling


class PyShepSegSubsetError(Exception):
    "Same name as the reference's exception (subset.py:450)"


class SubsetResult(object):
    """segimg: recoded window (newYsize, newXsize) uint32; origSegIds[new id] = old id (row 0 = 0);
    hist[new id] = pixel count (the output 'Histogram' column); columns: the input RAT columns
    gathered to the new ids (plus origSegIdColName when asked for).  From
    distributed.subsetImageDistributed: segimg holds window rows [rows[0], rows[1]) only."""
    def __init__(self):
        self.segimg = None
        self.origSegIds = None
        self.hist = None
        self.columns = {}
        self.rows = None        # subsetImageDistributed: (a, b), the window rows of segimg


def _load(x):
    if isinstance(x, str):
        if not x.endswith('.npy'):
            raise PyShepSegSubsetError("GDAL is not available here: pass a numpy array or a .npy path")
        return numpy.load(x, mmap_mode='r')
    return x


def subsetImage(inname, outname, tlx, tly, newXsize, newYsize, outformat=None, creationOptions=[],
                origSegIdColName=None, maskImage=None, ratColumns=None, tileSize=None):
    """
    Same arguments as the reference (subset.py:39-40) plus ``ratColumns`` (dict name -> array
    with one row per input segment id, the input RAT) and ``tileSize`` (visiting-order tile,
    default tiling.TILESIZE as in the reference).  ``inname`` is a (nRows, nCols) uint32 array
    or a ``.npy`` path; ``outname`` None (result only) or a ``.npy`` path; ``maskImage`` an
    array / ``.npy`` path of shape (newYsize, newXsize): only non-zero pixels are included.
    Returns a :class:`SubsetResult`.
    """
    seg = _load(inname)
    if seg.ndim != 2:
        raise PyShepSegSubsetError("input must be a single-band label raster")
    (tlx, tly, newXsize, newYsize) = (int(tlx), int(tly), int(newXsize), int(newYsize))
    checkWindow(seg.shape[0], seg.shape[1], tlx, tly, newXsize, newYsize)
    mask = loadMask(maskImage, newXsize, newYsize)
    if tileSize is None:
        tileSize = tiling.TILESIZE
    # only the window is needed on the device
    win = numpy.ascontiguousarray(seg[tly:tly + newYsize, tlx:tlx + newXsize], dtype=shepseg.SegIdType)
    valid = win if mask is None else win[mask != 0]
    valid = valid[valid != shepseg.SEGNULLVAL]
    if valid.size == 0:
        raise PyShepSegSubsetError('No valid data found in subset')
    maxId = int(valid.max())
    checkMaxId(maxId)
    cap = min(maxId, win.size) + 1
    out = numpy.empty((newYsize, newXsize), dtype=shepseg.SegIdType)
    orig = numpy.zeros(cap, dtype=numpy.uint32)
    hist = numpy.zeros(cap, dtype=numpy.uint32)
    nnew = ctypes.c_uint32(0)
    c = _lib.ctx()
    c.check(c._L.shp_subset_recode(
        c.handle, _lib.ptr(win), newYsize, newXsize, 0, 0, newXsize, newYsize,
        _lib.ptr(mask) if mask is not None else None, int(tileSize), maxId, _lib.ptr(out),
        _lib.ptr(orig), _lib.ptr(hist), cap, ctypes.byref(nnew)))
    n = nnew.value
    res = SubsetResult()
    res.segimg = out
    res.origSegIds = orig[:n + 1].copy()
    res.hist = hist[:n + 1].copy()
    res.columns = recodeColumns(res.origSegIds, res.hist, ratColumns, origSegIdColName)
    if outname is not None:
        checkOutname(outname)
        numpy.save(outname, out)
    return res


def checkWindow(nRows, nCols, tlx, tly, newXsize, newYsize):
    "the window must lie inside the nRows x nCols label raster (subset.py:86-88)"
    if (tlx + newXsize) > nCols or (tly + newYsize) > nRows or tlx < 0 or tly < 0:
        raise PyShepSegSubsetError('Requested subset is not within input image')


def loadMask(maskImage, newXsize, newYsize):
    """maskImage (None, an array or a .npy path) as contiguous uint8 0 / 1 of the window's shape, or None
    (subset.py:121-123)"""
    if maskImage is None:
        return None
    mask = numpy.asarray(_load(maskImage))
    if mask.shape != (newYsize, newXsize):
        raise PyShepSegSubsetError('mask should match requested subset size if supplied')
    return numpy.ascontiguousarray(mask != 0, dtype=numpy.uint8)


def checkMaxId(maxId):
    "the recode counts the ids 0..maxId in 32 bits, so the largest label a window may hold is 2^32 - 2"
    if maxId >= 0xffffffff:
        raise PyShepSegSubsetError('segment id %d in the subset is too large (at most %d)' % (maxId, 0xfffffffe))


def checkOutname(outname):
    if not (isinstance(outname, str) and outname.endswith('.npy')):
        raise PyShepSegSubsetError("GDAL is not available here: outname must be None or a .npy path")


def recodeColumns(origSegIds, hist, ratColumns, origSegIdColName):
    """The output RAT: every input column gathered to the new ids (copySubsettedSegmentsToNew,
    subset.py:232-266; row 0 = 0), 'Histogram' (:196-205) and origSegIdColName (:207-226).
    origSegIds[new id] = old id with at least one new id; returns a dict name -> array."""
    columns = {}
    maxId = int(origSegIds.max())
    if ratColumns:
        for name, col in ratColumns.items():
            col = numpy.asarray(col)
            if col.shape[0] <= maxId:
                raise PyShepSegSubsetError("RAT column %r has %d rows, segment id %d needs more"
                                           % (name, col.shape[0], maxId))
            new = col[origSegIds]
            new[0] = 0
            columns[name] = new
    columns['Histogram'] = hist.astype(numpy.float64)
    if origSegIdColName is not None:
        columns[origSegIdColName] = origSegIds.astype(numpy.int32)
    return columns
