"""Drop-in for the non-spatial part of ``pyshepseg.tilingstats``: per-segment statistics of an
image band against a segmentation raster, computed on the GPU.

``calcPerSegmentStatsTiled(imgfile, imgbandnum, segfile, statsSelection, missingStatsValue)``
keeps the reference signature (tilingstats.py:85-216).  The reference streams 1024² tiles
through numba dict-of-dict histograms and pages the results into the GDAL RAT; here the whole
band and label raster go to HBM once and the exact per-segment value multisets come out of two
stable radix sorts (``shp_segstats``).  Results are identical for the integer statistics and
bit-identical for mean / stddev on the reference's golden vectors.

Rasters: numpy arrays or ``.npy`` paths (GDAL optional, imported lazily).  Without GDAL the
columns are returned in ``result.columns`` (name -> array indexed by segment id) instead of
being written to the RAT.

Spatial statistics (``calcPerSegmentSpatialStatsTiled``, tilingstats.py:1262-1390): the reference's
three example user functions (``userFuncMeanCoord``, ``userFuncNumEdgePixels``,
``userFuncVariogram``) are fixed reductions on the GPU.  Any other ``userFunc(pts, imgNullVal,
intArr, floatArr, userParam)``, decorated with ``spatialUserFunc`` (the reference's @njit
requirement; @jit / @njit functions pass as they are), is called on the host once per segment with
that segment's points,
which the GPU groups by segment in the reference's visit order (``iterSegmentPoints``); segments
are called in ascending id order rather than in the reference's order of completion.  Out of
scope: the RIOS variants.
"""
import concurrent.futures
import contextlib
import ctypes

import numpy

from . import _lib
from . import shepseg
from .tiling import Timers, TILESIZE

STATID_MIN = 0
STATID_MAX = 1
STATID_MEAN = 2
STATID_STDDEV = 3
STATID_MEDIAN = 4
STATID_MODE = 5
STATID_PERCENTILE = 6
STATID_PIXCOUNT = 7
statIDdict = {'min': STATID_MIN, 'max': STATID_MAX, 'mean': STATID_MEAN, 'stddev': STATID_STDDEV,
              'median': STATID_MEDIAN, 'mode': STATID_MODE, 'percentile': STATID_PERCENTILE,
              'pixcount': STATID_PIXCOUNT}
STATSSELFAST_DTYPE = numpy.uint32
NOPARAM = numpy.iinfo(STATSSELFAST_DTYPE).max
STAT_DTYPE_INT = 0
STAT_DTYPE_FLOAT = 1
(STATSEL_GLOBALCOLINDEX, STATSEL_STATID, STATSEL_COLTYPE, STATSEL_COLARRAYINDEX,
 STATSEL_PARAM) = range(5)
RAT_PAGE_SIZE = 100000


class PyShepSegStatsError(Exception):
    pass


class TiledStatsResult(object):
    """Result of calcPerSegmentStatsTiled (reference tilingstats.py:219-232) plus the computed
    columns (name -> ndarray indexed by segment id; int64 or float32)."""
    def __init__(self):
        self.timings = None
        self.columns = None


def makeFastStatsSelection(colIndexList, statsSelection):
    """(statsSelection_fast, numIntCols, numFloatCols) exactly as the reference builds them
    (tilingstats.py:798-863)."""
    numStats = len(colIndexList)
    fast = numpy.empty((numStats, 5), dtype=STATSSELFAST_DTYPE)
    intCount = 0
    floatCount = 0
    for i in range(numStats):
        fast[i, STATSEL_GLOBALCOLINDEX] = colIndexList[i]
        statName = statsSelection[i][1]
        if statName not in statIDdict:
            raise PyShepSegStatsError("Unknown statistic '{}'".format(statName))
        fast[i, STATSEL_STATID] = statIDdict[statName]
        statType = STAT_DTYPE_FLOAT if statName in ('mean', 'stddev') else STAT_DTYPE_INT
        fast[i, STATSEL_COLTYPE] = statType
        if statType == STAT_DTYPE_INT:
            fast[i, STATSEL_COLARRAYINDEX] = intCount
            intCount += 1
        else:
            fast[i, STATSEL_COLARRAYINDEX] = floatCount
            floatCount += 1
        fast[i, STATSEL_PARAM] = NOPARAM
        if statName == 'percentile':
            fast[i, STATSEL_PARAM] = statsSelection[i][2]
    return (fast, intCount, floatCount)


def _loadArray(obj, band=None):
    if isinstance(obj, numpy.ndarray):
        arr = obj
    elif isinstance(obj, str) and obj.endswith('.npy'):
        arr = numpy.load(obj, mmap_mode='r')
    else:
        return None
    if band is not None and arr.ndim == 3:
        arr = arr[band - 1]
    return arr


def calcPerSegmentStats(seg, band, statsSelection, imgNullVal=None, missingStatsValue=-9999,
                        maxSegId=None):
    """The compute step on arrays: returns (intcols int64 (nInt, maxSegId+1), floatcols float32
    (nFloat, maxSegId+1), statsSelection_fast)."""
    seg = numpy.ascontiguousarray(seg, dtype=shepseg.SegIdType)
    band = numpy.ascontiguousarray(band)
    if band.dtype.kind == 'f':
        raise PyShepSegStatsError("Float image types not supported")      # tilingstats.py:450-452
    if band.dtype not in _lib.SHP_DTYPES:
        b3, _dt = _lib.as_image(band.reshape((1,) + band.shape))
        band = b3[0]
    if band.shape != seg.shape:
        raise PyShepSegStatsError("Images are different sizes")           # tilingstats.py:453-455
    if maxSegId is None:
        maxSegId = int(seg.max()) if seg.size else 0
    (fast, nInt, nFloat) = makeFastStatsSelection(list(range(len(statsSelection))), statsSelection)
    intcols = numpy.zeros((nInt, maxSegId + 1), dtype=numpy.int64)
    floatcols = numpy.zeros((nFloat, maxSegId + 1), dtype=numpy.float32)
    c = _lib.ctx()
    c.check(c._L.shp_segstats(c.handle, _lib.ptr(seg), _lib.ptr(band), _lib.SHP_DTYPES[band.dtype],
                              seg.size, maxSegId, int(imgNullVal is not None),
                              0 if imgNullVal is None else int(imgNullVal), _lib.ptr(fast),
                              len(statsSelection), int(missingStatsValue), _lib.ptr(intcols),
                              _lib.ptr(floatcols)))
    return intcols, floatcols, fast


# ------------------------------------------------------------------------------------------
# paged RAT (reference tilingstats.py:1935-2045, :723-764)
# ------------------------------------------------------------------------------------------
def getRatPageId(segId):
    """The page a segment id lives in = the id of the page's first row (tilingstats.py:1950-1956)."""
    return (int(segId) // RAT_PAGE_SIZE) * RAT_PAGE_SIZE


class RatPage(object):
    """One page of the paged RAT: RAT_PAGE_SIZE consecutive segment ids (fewer in the last page),
    int columns int64, float columns float32, a completion flag per row; the null segment's row
    is born complete, all zero (reference tilingstats.py:1972-2045)."""
    def __init__(self, numIntCols, numFloatCols, startSegId, numSeg):
        self.startSegId = int(startSegId)
        self.intcols = numpy.empty((numIntCols, numSeg), dtype=numpy.int64)
        self.floatcols = numpy.empty((numFloatCols, numSeg), dtype=numpy.float32)
        self.complete = numpy.zeros(numSeg, dtype=bool)
        if self.startSegId == shepseg.SEGNULLVAL:
            self.complete[0] = True
            self.intcols[:, 0] = 0
            self.floatcols[:, 0] = 0

    def getIndexInPage(self, segId):
        return segId - self.startSegId

    def setRatVal(self, segId, colType, colArrayNdx, val):
        if colType == STAT_DTYPE_INT:
            self.intcols[colArrayNdx, segId - self.startSegId] = val
        elif colType == STAT_DTYPE_FLOAT:
            self.floatcols[colArrayNdx, segId - self.startSegId] = val

    def getRatVal(self, segId, colType, colArrayNdx):
        if colType == STAT_DTYPE_INT:
            return self.intcols[colArrayNdx, segId - self.startSegId]
        return self.floatcols[colArrayNdx, segId - self.startSegId]

    def setSegmentComplete(self, segId):
        self.complete[segId - self.startSegId] = True

    def getSegmentComplete(self, segId):
        return bool(self.complete[segId - self.startSegId])

    def pageComplete(self):
        return bool(self.complete.all())


def createPagedRat():
    """page id -> RatPage, initially empty (reference tilingstats.py:1935-1946)."""
    return {}


class MemoryRat(object):
    """Stands where the reference has the GDAL RasterAttributeTable when the rasters are arrays:
    the same ``WriteArray(column, colNumber, start=row)`` call fills whole-table column arrays
    (``columns[colNumber]``, int64 or float32, numRows rows).  ``pagesWritten`` records the
    (startSegId, numRows) of every page in the order it was written."""
    def __init__(self, numRows, colTypes):
        self.columns = [numpy.zeros(numRows, dtype=numpy.float32 if t == STAT_DTYPE_FLOAT else numpy.int64)
                        for t in colTypes]
        self.pagesWritten = []

    def WriteArray(self, colArr, colNumber, start=0):
        self.columns[colNumber][start:start + len(colArr)] = colArr

    def notePage(self, startSegId, numRows):
        self.pagesWritten.append((int(startSegId), int(numRows)))


def writeCompletePages(pagedRat, attrTbl, statsSelection_fast):
    """Write every completed page to the attribute table, column by column at its start row, and
    drop it from the paged RAT (reference tilingstats.py:723-764)."""
    for pageId in sorted(pagedRat.keys()):
        ratPage = pagedRat[pageId]
        if not ratPage.pageComplete():
            continue
        for statSel in statsSelection_fast:
            colNumber = int(statSel[STATSEL_GLOBALCOLINDEX])
            if statSel[STATSEL_COLTYPE] == STAT_DTYPE_INT:
                colArr = ratPage.intcols[statSel[STATSEL_COLARRAYINDEX]]
            else:
                colArr = ratPage.floatcols[statSel[STATSEL_COLARRAYINDEX]]
            attrTbl.WriteArray(colArr, colNumber, start=ratPage.startSegId)
        if hasattr(attrTbl, 'notePage'):
            attrTbl.notePage(ratPage.startSegId, len(ratPage.complete))
        pagedRat.pop(pageId)


def _pageRows(pagedRat, segIds, intRows, floatRows, segSize, numIntCols, numFloatCols, emptyRow):
    """Store finished rows (columns x ids) in their pages and flag them complete.  A page is created
    on first touch; ids of that page which have no pixels at all (segSize == 0: the stitch can
    leave such ids, tiling.py:1308-1341) are completed there and then with `emptyRow`, so that the
    page can finish -- the reference never sees them and fails with 'Not all pixels found'."""
    if len(segIds) == 0:
        return
    numRows = len(segSize)
    pages = (segIds // RAT_PAGE_SIZE) * RAT_PAGE_SIZE
    order = numpy.argsort(pages, kind='stable')
    (upages, first) = numpy.unique(pages[order], return_index=True)
    bounds = list(first) + [len(order)]
    for (k, pageId) in enumerate(upages):
        sel = order[bounds[k]:bounds[k + 1]]
        pageId = int(pageId)
        page = pagedRat.get(pageId)
        if page is None:
            numSeg = min(RAT_PAGE_SIZE, numRows - pageId)
            page = pagedRat[pageId] = RatPage(numIntCols, numFloatCols, pageId, numSeg)
            empty = numpy.flatnonzero(segSize[pageId:pageId + numSeg] == 0)
            if pageId == shepseg.SEGNULLVAL:
                empty = empty[empty != 0]                     # row 0 is the null segment: zeros
            if len(empty):
                page.intcols[:, empty] = emptyRow[0][:, None]
                page.floatcols[:, empty] = emptyRow[1][:, None]
                page.complete[empty] = True
        idx = segIds[sel] - pageId
        page.intcols[:, idx] = intRows[:, sel]
        page.floatcols[:, idx] = floatRows[:, sel]
        page.complete[idx] = True


class _ChunkSource(object):
    """Row blocks of (label raster, image planes) as device pointers: resident rasters are addressed in
    place, host arrays / memmaps go up block by block into reusable device buffers.  planes: host planes
    (arrays / memmaps), or devPlanes: device addresses of whole planes."""
    def __init__(self, c, seg, planes, devSeg=None, devPlanes=None, bandDtype=None, shape=None):
        self.c = c
        (self.seg, self.planes, self.devSeg, self.devPlanes) = (seg, planes, devSeg, devPlanes)
        self.nplanes = len(planes if devPlanes is None else devPlanes)
        (self.nrows, self.ncols) = shape
        self.bandDtype = numpy.dtype(bandDtype)
        self.bufs = []

    def _buf(self, i, nbytes):
        while len(self.bufs) <= i:
            self.bufs.append([None, 0])
        if self.bufs[i][1] < nbytes:
            if self.bufs[i][0] is not None:
                self.c.check(self.c._L.shp_dev_free(self.c.handle, self.bufs[i][0]))
            p = ctypes.c_void_p()
            self.c.check(self.c._L.shp_dev_alloc(self.c.handle, nbytes, ctypes.byref(p)))
            self.bufs[i] = [p, nbytes]
        return self.bufs[i][0]

    def chunk(self, y0, y1):
        """(labels, [one pointer per plane]) of rows y0..y1"""
        n = (y1 - y0) * self.ncols
        isz = self.bandDtype.itemsize
        if self.devSeg is not None:
            return (ctypes.c_void_p(self.devSeg + 4 * y0 * self.ncols),
                    [ctypes.c_void_p(p + isz * y0 * self.ncols) for p in self.devPlanes])
        s = numpy.ascontiguousarray(self.seg[y0:y1], dtype=shepseg.SegIdType)
        ds = self._buf(0, n * 4)
        self.c.check(self.c._L.shp_dev_upload(self.c.handle, ds, _lib.ptr(s), s.nbytes))
        dbs = []
        for (k, plane) in enumerate(self.planes):
            b = numpy.ascontiguousarray(plane[y0:y1], dtype=self.bandDtype)
            db = self._buf(3 + k, n * isz)
            self.c.check(self.c._L.shp_dev_upload(self.c.handle, db, _lib.ptr(b), b.nbytes))
            dbs.append(db)
        return (ds, dbs)

    def scratch(self, i, nbytes):
        return self._buf(1 + i, nbytes)             # (buffers 1 and 2; the planes' start at 3)

    def close(self):
        for (p, _n) in self.bufs:
            if p is not None:
                self.c.check(self.c._L.shp_dev_free(self.c.handle, p))
        self.bufs = []


STATS_CHUNK_PIXELS = 1 << 28        # pixels per streamed block (the kernels index a block with 32 bits)


def _streamStats(src, entries, segSize, statsSelection_fast, missingStatsValue, attrTbl, timings, chunkPixels):
    """The tile loop of calcPerSegmentStatsTiled (tilingstats.py:183-206) over row blocks, for one band or several:
    ``entries`` is a list of (plane of src, null value, statsSelection), ``statsSelection_fast`` the combined fast
    selection of their statsSelections one after the other.  Per block: the labels are renumbered 1..m in first-seen
    order on the device (the subset module's recode, which also counts their pixels), all entries' statistics are computed
    for those m ids, the ids whose block count equals segSize are complete (checkSegComplete, :518-553) and go to
    their RAT page -- a property of the labels, established once; the pixels of the others are set aside as ids once
    and one value array per plane, in one order, and reduced per entry at the end.
    One entry goes through the one-band library calls (k_stats_patch), several through the bands calls
    (k_stats_patch_bands): csrc/segstats.h has why these are two kernels."""
    c = src.c
    L = c._L
    (nrows, ncols) = (src.nrows, src.ncols)
    S = len(segSize) - 1
    dt = _lib.SHP_DTYPES[src.bandDtype]
    nEntries = len(entries)
    fast = numpy.ascontiguousarray(statsSelection_fast, dtype=numpy.uint32)
    numIntCols = int((fast[:, STATSEL_COLTYPE] == STAT_DTYPE_INT).sum())
    numFloatCols = len(fast) - numIntCols
    planeOfEntry = [e[0] for e in entries]
    perBand = numpy.ascontiguousarray([len(e[2]) for e in entries], dtype=numpy.int32)
    bandOfStat = numpy.repeat(numpy.arange(nEntries), perBand)
    hasNull = numpy.ascontiguousarray([int(e[1] is not None) for e in entries], dtype=numpy.int32)
    nullArr = numpy.ascontiguousarray([0 if e[1] is None else int(e[1]) for e in entries], dtype=numpy.int64)
    # statistics of a segment without pixels (see _pageRows)
    emptyInt = numpy.full(numIntCols, int(missingStatsValue), dtype=numpy.int64)
    emptyFloat = numpy.full(numFloatCols, float(missingStatsValue), dtype=numpy.float32)
    for sel in fast:
        if sel[STATSEL_STATID] == STATID_PIXCOUNT:
            emptyInt[sel[STATSEL_COLARRAYINDEX]] = 0
    pagedRat = createPagedRat()
    written = set()

    def flush():
        written.update(pid for (pid, pg) in pagedRat.items() if pg.pageComplete())
        writeCompletePages(pagedRat, attrTbl, fast)

    def pointers(planes, which):
        arr = (ctypes.c_void_p * len(which))()
        for (k, p) in enumerate(which):
            arr[k] = planes[p].value
        return arr

    def blockStats(drec, dplanes, blockRows, m, ic, fc):
        """the statistics of all entries for the block's ids 1..m"""
        if nEntries == 1:
            # (the block's shape goes along: with small segments the library works patch by patch)
            c.check(L.shp_segstats2d_dev(c.handle, drec, dplanes[planeOfEntry[0]], dt, blockRows, ncols, m,
                                         int(hasNull[0]), int(nullArr[0]), _lib.ptr(fast), len(fast),
                                         int(missingStatsValue), _lib.ptr(ic), _lib.ptr(fc)))
        else:
            c.check(L.shp_segstats2d_bands_dev(c.handle, drec, pointers(dplanes, planeOfEntry), dt, nEntries,
                                               blockRows, ncols, m, _lib.ptr(hasNull), _lib.ptr(nullArr),
                                               _lib.ptr(fast), _lib.ptr(perBand), int(missingStatsValue),
                                               _lib.ptr(ic), _lib.ptr(fc)))

    def gatherFlagged(drec, dplanes, n, m, flags, npairs):
        """(ids, values[plane]) of the npairs pixels of the block whose id is flagged"""
        so = numpy.empty(npairs, dtype=numpy.uint32)
        vo = numpy.empty((src.nplanes, npairs), dtype=numpy.int64)
        cnt = ctypes.c_int64(0)
        if nEntries == 1:                                   # (one entry reads one plane)
            c.check(L.shp_gather_flagged_dev(c.handle, drec, dplanes[0], dt, n, m, _lib.ptr(flags), npairs,
                                             _lib.ptr(so), _lib.ptr(vo), ctypes.byref(cnt)))
        else:
            c.check(L.shp_gather_flagged_bands_dev(c.handle, drec, pointers(dplanes, range(src.nplanes)), dt,
                                                   src.nplanes, n, m, _lib.ptr(flags), npairs, _lib.ptr(so),
                                                   _lib.ptr(vo), ctypes.byref(cnt)))
        if cnt.value != npairs:
            raise PyShepSegStatsError("internal: %d pixels of unfinished segments, expected %d"
                                      % (cnt.value, npairs))
        return (so, vo)

    rowsPerChunk = max(1, min(nrows, int(chunkPixels) // max(ncols, 1)))
    carryIds = []
    carryVals = []
    for y0 in range(0, nrows, rowsPerChunk):
        y1 = min(nrows, y0 + rowsPerChunk)
        n = (y1 - y0) * ncols
        with timings.interval('reading'):
            (dseg, dplanes) = src.chunk(y0, y1)
        with timings.interval('accumulation'):
            cap = min(S, n) + 1
            drec = src.scratch(0, n * 4)
            orig = numpy.zeros(cap, dtype=numpy.uint32)
            lhist = numpy.zeros(cap, dtype=numpy.uint32)
            nnew = ctypes.c_uint32(0)
            c.check(L.shp_subset_recode_dev(c.handle, dseg, y1 - y0, ncols, 0, 0, ncols, y1 - y0, None,
                                            1 << 30, S, drec, _lib.ptr(orig), _lib.ptr(lhist), cap,
                                            ctypes.byref(nnew)))
            m = nnew.value
            if m == 0:
                continue
            ic = numpy.zeros((max(numIntCols, 1), m + 1), dtype=numpy.int64)
            fc = numpy.zeros((max(numFloatCols, 1), m + 1), dtype=numpy.float32)
            blockStats(drec, dplanes, y1 - y0, m, ic, fc)
        with timings.interval('statscompletion'):
            ids = orig[1:m + 1].astype(numpy.int64)
            done = lhist[1:m + 1] == segSize[ids]
            sel = numpy.flatnonzero(done)
            _pageRows(pagedRat, ids[sel], ic[:numIntCols, 1:][:, sel], fc[:numFloatCols, 1:][:, sel],
                      segSize, numIntCols, numFloatCols, (emptyInt, emptyFloat))
            rest = numpy.flatnonzero(~done)
            if len(rest):
                flags = numpy.zeros(m + 1, dtype=numpy.uint8)
                flags[rest + 1] = 1
                (so, vo) = gatherFlagged(drec, dplanes, n, m, flags, int(lhist[1:m + 1][rest].sum()))
                carryIds.append(orig[so])
                carryVals.append(vo.astype(src.bandDtype))
        with timings.interval('writing'):
            flush()
    if carryIds:
        # the segments that straddle block boundaries: all their pixels are here now
        with timings.interval('statscompletion'):
            allIds = numpy.concatenate(carryIds)
            allVals = numpy.concatenate(carryVals, axis=1)
            (uids, compact) = numpy.unique(allIds, return_inverse=True)
            counts = numpy.bincount(compact, minlength=len(uids))
            if not numpy.array_equal(counts, segSize[uids]):
                raise PyShepSegStatsError('Not all pixels found during processing')     # tilingstats.py:211
            m = len(uids)
            ic = numpy.zeros((max(numIntCols, 1), m + 1), dtype=numpy.int64)
            fc = numpy.zeros((max(numFloatCols, 1), m + 1), dtype=numpy.float32)
            seg1 = numpy.ascontiguousarray(compact + 1, dtype=numpy.uint32)
            for (k, (plane, _nullVal, statsSelection)) in enumerate(entries):
                # (shp_segstats numbers its columns from 0: the entry's own fast selection; with one entry that
                #  is the combined one)
                (bfast, bInt, bFloat) = makeFastStatsSelection(list(range(len(statsSelection))), statsSelection)
                bic = numpy.zeros((max(bInt, 1), m + 1), dtype=numpy.int64)
                bfc = numpy.zeros((max(bFloat, 1), m + 1), dtype=numpy.float32)
                vals = numpy.ascontiguousarray(allVals[plane])
                c.check(L.shp_segstats(c.handle, _lib.ptr(seg1), _lib.ptr(vals), dt, len(seg1), m,
                                       int(hasNull[k]), int(nullArr[k]), _lib.ptr(bfast), len(bfast),
                                       int(missingStatsValue), _lib.ptr(bic), _lib.ptr(bfc)))
                for (own, comb) in zip(bfast, fast[bandOfStat == k]):
                    if own[STATSEL_COLTYPE] == STAT_DTYPE_INT:
                        ic[comb[STATSEL_COLARRAYINDEX]] = bic[own[STATSEL_COLARRAYINDEX]]
                    else:
                        fc[comb[STATSEL_COLARRAYINDEX]] = bfc[own[STATSEL_COLARRAYINDEX]]
            _pageRows(pagedRat, uids.astype(numpy.int64), ic[:numIntCols, 1:], fc[:numFloatCols, 1:], segSize,
                      numIntCols, numFloatCols, (emptyInt, emptyFloat))
    # pages no block touched hold only ids without pixels
    with timings.interval('writing'):
        for pageId in range(0, S + 1, RAT_PAGE_SIZE):
            if pageId in written or pageId in pagedRat:
                continue
            if (segSize[max(pageId, 1):pageId + RAT_PAGE_SIZE] != 0).any():
                raise PyShepSegStatsError('Not all pixels found during processing')      # tilingstats.py:211
            numSeg = min(RAT_PAGE_SIZE, S + 1 - pageId)
            page = pagedRat[pageId] = RatPage(numIntCols, numFloatCols, pageId, numSeg)
            first = 1 if pageId == shepseg.SEGNULLVAL else 0
            page.intcols[:, first:] = emptyInt[:, None]
            page.floatcols[:, first:] = emptyFloat[:, None]
            page.complete[:] = True
        flush()
    if len(pagedRat) > 0:
        raise PyShepSegStatsError('Not all pixels found during processing')              # tilingstats.py:211


def _planeNumbers(bandSelections):
    """The band numbers whose planes a call reads, ascending: a band listed twice is read once."""
    return sorted(set(b for (b, _s) in bandSelections))


def _tiledStats(imgfile, hostPlanes, segfile, bandSelections, statsSelection_fast, nullVals, missingStatsValue,
                segSize, chunkPixels):
    """What calcPerSegmentStatsTiled and calcPerSegmentStatsTiledBands share: the rasters resolved to a block
    source (a device raster with resident labels; arrays / .npy; GDAL files), segSize, the attribute table, the
    streaming loop, the result.  bandSelections: a list of (imgbandnum, statsSelection), statsSelection_fast their
    combined fast selection (None: built here with makeFastStatsSelection, once the rasters are open).
    hostPlanes: the 2-D planes of _planeNumbers(bandSelections) when the caller found imgfile to be an array or a
    .npy path, else None.  nullVals(default): the null value of every entry, given
    every entry's default (the raster's / its band's own nodata value, None on arrays)."""
    timings = Timers()
    from . import tiling as _tiling
    flatSelection = [sel for (_b, s) in bandSelections for sel in s]
    bandNums = [b for (b, _s) in bandSelections]
    planes = _planeNumbers(bandSelections)
    planeOfEntry = [planes.index(b) for b in bandNums]
    c = _lib.ctx()
    gdalSeg = None
    if chunkPixels is None:
        chunkPixels = STATS_CHUNK_PIXELS
    with timings.interval('reading'):
        if isinstance(imgfile, _tiling.DeviceRaster) and getattr(segfile, 'outDev', None):
            (dptr, nrows, ncols, _nbytes) = segfile.outDev
            (nb, ir, ic_) = imgfile.shape
            if (ir, ic_) != (nrows, ncols):
                raise PyShepSegStatsError("Images are different sizes")
            for b in bandNums:
                if not (1 <= b <= nb):
                    raise PyShepSegStatsError("band %d not in image" % b)
            nullVals = nullVals([imgfile.nullVal] * len(bandNums))
            if segSize is None:
                segSize = getattr(segfile, 'hist', None)
            devPlanes = [imgfile.ptr + (b - 1) * nrows * ncols * imgfile.dtype.itemsize for b in planes]
            src = _ChunkSource(c, None, None, devSeg=dptr, devPlanes=devPlanes, bandDtype=imgfile.dtype,
                               shape=(nrows, ncols))
            maxSegId = int(segfile.maxSegId)
        else:
            seg = _loadArray(segfile)
            if seg is None or hostPlanes is None:
                (seg, hostPlanes, nodata, gdalSeg, segSize) = _readGdalBands(imgfile, planes, segfile)
                nullVals = nullVals([nodata[p] for p in planeOfEntry])
            else:
                nullVals = nullVals([None] * len(bandNums))
            if hostPlanes[0].dtype.kind == 'f':
                raise PyShepSegStatsError("Float image types not supported")        # tilingstats.py:450-452
            if hostPlanes[0].shape != seg.shape:
                raise PyShepSegStatsError("Images are different sizes")             # tilingstats.py:453-455
            bdt = hostPlanes[0].dtype
            if bdt not in _lib.SHP_DTYPES:
                bdt = _lib.as_image(numpy.zeros((1, 1, 1), dtype=bdt))[0].dtype
            src = _ChunkSource(c, seg, hostPlanes, bandDtype=bdt, shape=seg.shape)
            maxSegId = None
    try:
        if segSize is None:
            with timings.interval('reading'):
                segSize = _countSegments(src, chunkPixels)
        segSize = numpy.ascontiguousarray(segSize).astype(numpy.int64)
        if maxSegId is not None and len(segSize) < maxSegId + 1:
            raise PyShepSegStatsError("segSize has %d rows, segment id %d needs more" % (len(segSize), maxSegId))
        fast = statsSelection_fast
        if fast is None:
            fast = makeFastStatsSelection(list(range(len(flatSelection))), flatSelection)[0]
        if gdalSeg is not None:
            attrTbl = _GdalRat(gdalSeg, flatSelection, fast)
        else:
            attrTbl = MemoryRat(len(segSize), [int(f[STATSEL_COLTYPE]) for f in fast])
        entries = [(planeOfEntry[k], nullVals[k], s) for (k, (_b, s)) in enumerate(bandSelections)]
        _streamStats(src, entries, segSize, fast, missingStatsValue, attrTbl, timings, chunkPixels)
    finally:
        src.close()
    rtn = TiledStatsResult()
    rtn.timings = timings
    if isinstance(attrTbl, MemoryRat):
        rtn.columns = {sel[0]: attrTbl.columns[i] for (i, sel) in enumerate(flatSelection)}
        rtn.pagesWritten = attrTbl.pagesWritten
    else:
        attrTbl.flush()
        rtn.columns = None
    return rtn


def calcPerSegmentStatsTiled(imgfile, imgbandnum, segfile, statsSelection,
        missingStatsValue=-9999, imgNullVal=None, segSize=None, chunkPixels=None):
    """
    Calculate selected per-segment statistics for the given band of imgfile against the
    segment raster segfile (reference tilingstats.py:85-216).  statsSelection is a list of
    (columnName, statName[, parameter]) with statName in 'min', 'max', 'mean', 'stddev',
    'median', 'mode', 'percentile', 'pixcount'.  Returns a TiledStatsResult whose ``columns``
    maps column name -> whole-table array; with GDAL files the columns are written to the
    segfile's RAT page by page (RAT_PAGE_SIZE rows) as the reference does.

    The rasters are streamed through the GPU in row blocks of ``chunkPixels`` pixels (default
    STATS_CHUNK_PIXELS), so they may be larger than the kernels' 32-bit pixel index and than HBM;
    a finished page leaves for the attribute table as soon as all its segments are complete.
    ``segSize`` stands for the reference's RAT 'Histogram' column (pixels per segment id): taken
    from the RAT for GDAL files, from ``segfile.hist`` for a tiled-segmentation result, counted
    here otherwise.  Both rasters may already live in HBM: ``imgfile`` a ``tiling.DeviceRaster``
    and ``segfile`` the result of ``doTiledShepherdSegmentation(..., outfile=tiling._KEEP_ON_DEVICE)``.
    """
    # (the selection may name a column twice or be empty -- makeBandStatsSelection refuses both, so it is not used
    #  here -- and the plane of an array is whatever _loadArray picks for imgbandnum)
    img = _loadArray(imgfile, imgbandnum)
    return _tiledStats(imgfile, None if img is None else [img], segfile, [(imgbandnum, statsSelection)], None,
                       lambda default: [default[0] if imgNullVal is None else imgNullVal],
                       missingStatsValue, segSize, chunkPixels)


def _countSegments(src, chunkPixels):
    """Pixels per segment id of the label raster (what the reference reads from the RAT's
    'Histogram' column, tilingstats.py:165-166), block by block on the device."""
    c = src.c
    (nrows, ncols) = (src.nrows, src.ncols)
    rowsPerChunk = max(1, min(max(nrows, 1), int(chunkPixels) // max(ncols, 1)))
    maxId = 0
    parts = []
    for y0 in range(0, nrows, rowsPerChunk):
        y1 = min(nrows, y0 + rowsPerChunk)
        if src.devSeg is None:
            blk = numpy.asarray(src.seg[y0:y1])
            parts.append(numpy.bincount(blk.reshape(-1)))
        else:
            raise PyShepSegStatsError("segSize (the label histogram) is needed for a device-resident label raster")
    n = max([len(p) for p in parts] or [1])
    out = numpy.zeros(n, dtype=numpy.int64)
    for p in parts:
        out[:len(p)] += p
    return out


# ------------------------------------------------------------------------------------------
# several bands against the same segmentation in one pass over the labels
# ------------------------------------------------------------------------------------------
def makeBandStatsSelection(bandSelections):
    """The combined fast selection of ``bandSelections``, a list of (imgbandnum, statsSelection):
    returns (fast, bandOfStat, numIntCols, numFloatCols), ``fast`` as makeFastStatsSelection gives it
    for the statsSelections one after the other (the global column index and the per-type column
    array index run through all entries), ``bandOfStat[i]`` the index of the bandSelections entry
    that statistic i belongs to.  Column names must be unique over all entries and every
    statsSelection non-empty."""
    bandSelections = list(bandSelections)
    if len(bandSelections) == 0:
        raise PyShepSegStatsError("bandSelections must hold one or more (imgbandnum, statsSelection)")
    flat = []
    bandOfStat = []
    names = set()
    for (k, entry) in enumerate(bandSelections):
        if len(entry) != 2:
            raise PyShepSegStatsError("bandSelections entry {} is not (imgbandnum, statsSelection)".format(k))
        statsSelection = list(entry[1])
        if len(statsSelection) == 0:
            raise PyShepSegStatsError("bandSelections entry {} (band {}) selects no statistic".format(k, entry[0]))
        for sel in statsSelection:
            if sel[0] in names:
                raise PyShepSegStatsError("Column name '{}' is used more than once".format(sel[0]))
            names.add(sel[0])
            flat.append(sel)
            bandOfStat.append(k)
    (fast, nInt, nFloat) = makeFastStatsSelection(list(range(len(flat))), flat)
    return (fast, numpy.array(bandOfStat, dtype=numpy.intp), nInt, nFloat)


def _entryNullVals(imgNullVal, nEntries, default):
    """One null value per bandSelections entry: imgNullVal is one value for all, a list with one entry
    each, or None (then default[k])."""
    if imgNullVal is None:
        return list(default)
    if isinstance(imgNullVal, (list, tuple, numpy.ndarray)):
        if len(imgNullVal) != nEntries:
            raise PyShepSegStatsError("imgNullVal has %d entries, bandSelections %d" % (len(imgNullVal), nEntries))
        return [default[k] if v is None else v for (k, v) in enumerate(imgNullVal)]
    return [imgNullVal] * nEntries


def calcPerSegmentStatsTiledBands(imgfile, bandSelections, segfile, missingStatsValue=-9999,
        imgNullVal=None, segSize=None, chunkPixels=None):
    """
    calcPerSegmentStatsTiled for several bands of imgfile in one pass over the segment raster:
    ``bandSelections`` is a list of (imgbandnum, statsSelection), each statsSelection as
    calcPerSegmentStatsTiled takes it; a band may appear in more than one entry, column names must be
    unique over the whole call.  ``imgNullVal`` is one value for all entries or a list with one per
    entry (GDAL files: each band's own nodata value when not given); a pixel that is null in one
    band still counts in the others.  Everything else -- the raster forms accepted, ``segSize``,
    ``chunkPixels``, the errors -- is as for calcPerSegmentStatsTiled, and every column is
    bit-identical to what that function returns for the entry's band and selection on its own.

    The label raster is read, uploaded, renumbered and histogrammed once per row block instead of once
    per band, and the patches' label tables are built once (csrc/segstats.h, k_stats_patch_bands).
    """
    (fast, _bandOfStat, _nInt, _nFloat) = makeBandStatsSelection(bandSelections)    # (the checks: before anything is read)
    bandSelections = [(int(b), list(s)) for (b, s) in bandSelections]
    img = _loadArray(imgfile)
    hostPlanes = None
    if img is not None:
        if img.ndim == 3:
            for (b, _s) in bandSelections:
                if not (1 <= b <= img.shape[0]):
                    raise PyShepSegStatsError("band %d not in image" % b)
            hostPlanes = [img[b - 1] for b in _planeNumbers(bandSelections)]
        else:
            hostPlanes = [img for _b in _planeNumbers(bandSelections)]     # (a single plane stands for any band, as _loadArray has it)
    return _tiledStats(imgfile, hostPlanes, segfile, bandSelections, fast,
                       lambda default: _entryNullVals(imgNullVal, len(bandSelections), default),
                       missingStatsValue, segSize, chunkPixels)


def _readGdalBands(imgfile, bandnums, segfile):
    """The reference's doImageAlignmentChecks + Histogram column read (tilingstats.py:151-166, :409-461) for the
    bands bandnums of imgfile; returns (seg, bands, each band's nodata value, segment dataset, segSize)."""
    try:
        from osgeo import gdal
    except ImportError:
        raise PyShepSegStatsError("GDAL (osgeo) is not importable here: pass numpy arrays or "
                                  ".npy paths")
    gdal.UseExceptions()
    segds = segfile if isinstance(segfile, gdal.Dataset) else gdal.Open(segfile, gdal.GA_Update)
    imgds = gdal.Open(imgfile)
    if (segds.RasterXSize != imgds.RasterXSize) or (segds.RasterYSize != imgds.RasterYSize):
        raise PyShepSegStatsError("Images are different sizes")
    if segds.GetGeoTransform() != imgds.GetGeoTransform():
        raise PyShepSegStatsError("Images have different spatial extents or pixel sizes")
    for b in bandnums:
        if not (1 <= b <= imgds.RasterCount):
            raise PyShepSegStatsError("band %d not in image" % b)
    imgbands = [imgds.GetRasterBand(b) for b in bandnums]
    attrTbl = segds.GetRasterBand(1).GetDefaultRAT()
    names = [attrTbl.GetNameOfCol(i) for i in range(attrTbl.GetColumnCount())]
    if 'Histogram' not in names:
        raise PyShepSegStatsError("Histogram column must exist before calculating per-segment stats")
    segSize = attrTbl.ReadAsArray(names.index('Histogram')).astype(numpy.uint32)
    return (segds.GetRasterBand(1).ReadAsArray(), [b.ReadAsArray() for b in imgbands],
            [b.GetNoDataValue() for b in imgbands], segds, segSize)


class _GdalRat(object):
    """The segfile's GDAL attribute table behind the WriteArray interface writeCompletePages uses;
    creates the requested columns like the reference's createStatColumns (tilingstats.py:682-720):
    Real for mean / stddev, Integer otherwise."""
    def __init__(self, segds, statsSelection, fast):
        from osgeo import gdal
        self.segds = segds
        self.tbl = segds.GetRasterBand(1).GetDefaultRAT()
        names = [self.tbl.GetNameOfCol(i) for i in range(self.tbl.GetColumnCount())]
        self.colNdx = []
        for sel in statsSelection:
            (colName, statName) = sel[:2]
            if colName not in names:
                colType = gdal.GFT_Real if statName in ('mean', 'stddev') else gdal.GFT_Integer
                self.tbl.CreateColumn(colName, colType, gdal.GFU_Generic)
                names.append(colName)
            else:
                print('Column {} already exists'.format(colName))
            self.colNdx.append(names.index(colName))

    def WriteArray(self, colArr, colNumber, start=0):
        self.tbl.WriteArray(colArr, self.colNdx[colNumber], start=start)

    def flush(self):
        self.segds.FlushCache()


# ------------------------------------------------------------------------------------------
# spatial statistics with the reference's built-in user functions
# ------------------------------------------------------------------------------------------
GFT_Integer, GFT_Real = 0, 1        # gdal.GFT_* values, so callers need not import GDAL


class _BuiltinSpatialFunc(object):
    """Stands for one of the reference's njit user functions; on the GPU they are fixed
    reductions (pyshepseg_amd/csrc/spatial.h), so the object only carries an id."""
    def __init__(self, funcId, name):
        self.funcId, self.__name__ = funcId, name

    def __call__(self, *args):
        raise PyShepSegStatsError("%s is evaluated on the GPU; it cannot be called" % self.__name__)


userFuncMeanCoord = _BuiltinSpatialFunc(0, 'userFuncMeanCoord')             # tilingstats.py:1098
userFuncNumEdgePixels = _BuiltinSpatialFunc(1, 'userFuncNumEdgePixels')     # tilingstats.py:1146
userFuncVariogram = _BuiltinSpatialFunc(2, 'userFuncVariogram')             # tilingstats.py:1037

def spatialUserFunc(func):
    """Decorator: marks a plain Python callable ``func(pts, imgNullVal, intArr, floatArr, userParam)``
    as a spatial user function for calcPerSegmentSpatialStats(Tiled).  It stands where the
    reference requires @jit / @njit (tilingstats.py:1330-1331: an undecorated callable is refused);
    numba-decorated functions are accepted as they are.  Returns ``func`` itself, or a wrapper when
    ``func`` takes no attributes."""
    try:
        func.shepsegSpatialUserFunc = True
        return func
    except AttributeError:
        def wrapper(*args):
            return func(*args)
        wrapper.shepsegSpatialUserFunc = True
        wrapper.__name__ = getattr(func, '__name__', 'userFunc')
        return wrapper


def _isUserFunc(userFunc):
    """A callable marked by spatialUserFunc, or a numba dispatcher (the reference's own test)."""
    return callable(userFunc) and (getattr(userFunc, 'shepsegSpatialUserFunc', False) is True or
                                   'targetoptions' in getattr(userFunc, '__dict__', {}))


# one point of a segment: the reference's SegPoint (tilingstats.py:1225-1240), column x and row y of the whole
# image, val widened to numbaTypeForImageType (int64)
SEGPOINT_DTYPE = numpy.dtype([('x', numpy.uint32), ('y', numpy.uint32), ('val', numpy.int64)])
POINTS_BATCH = 1 << 24              # default points per batch of iterSegmentPoints (256 MiB of records)


def _spatialArrays(seg, band):
    """(seg uint32, band in a library dtype), both C-contiguous 2-D and of one shape."""
    seg = numpy.ascontiguousarray(seg, dtype=shepseg.SegIdType)
    band = numpy.ascontiguousarray(band)
    if band.dtype.kind == 'f':
        raise PyShepSegStatsError("Float image types not supported")
    if band.dtype not in _lib.SHP_DTYPES:
        b3, _dt = _lib.as_image(band.reshape((1,) + band.shape))
        band = b3[0]
    if band.shape != seg.shape or seg.ndim != 2:
        raise PyShepSegStatsError("Images are different sizes")
    return seg, band


class _PinnedBuffer(object):
    """Pinned host memory of a context.  Arrays over it keep it (and so the context) alive: it is freed when
    the last of them goes, not when the generator that filled it ends."""
    def __init__(self, c, nbytes):
        self.c = c
        self.p = ctypes.c_void_p()
        c.check(c._L.shp_host_alloc(c.handle, nbytes, ctypes.byref(self.p)))

    def points(self, n):
        raw = (ctypes.c_uint8 * (n * SEGPOINT_DTYPE.itemsize)).from_address(self.p.value)
        raw._owner = self
        pts = numpy.frombuffer(raw, dtype=SEGPOINT_DTYPE).view(numpy.recarray)
        pts.flags.writeable = False
        return pts

    def __del__(self):
        if self.p.value and self.c.handle is not None:
            self.c._L.shp_host_free(self.c.handle, self.p)
            self.p = ctypes.c_void_p()


def planPointBatches(counts, batchPoints, idLo=1, idHi=None):
    """Split the ids [idLo, idHi) (idHi defaults to len(counts)) into consecutive ranges (lo, hi) whose
    points (counts[id] each) add up to at most batchPoints.  A segment with more points than that gets a
    range of its own.  Every id lies in exactly one range, the ranges in ascending order."""
    counts = numpy.asarray(counts, dtype=numpy.int64)
    if idHi is None:
        idHi = len(counts)
    batchPoints = max(1, int(batchPoints))
    cum = numpy.zeros(max(idHi - idLo, 0) + 1, dtype=numpy.int64)
    numpy.cumsum(counts[idLo:idHi], out=cum[1:])
    ranges = []
    start = 0
    nIds = len(cum) - 1
    while start < nIds:
        # the last end whose batch [start, end) keeps within the budget (ids without points ride along)
        end = int(numpy.searchsorted(cum, cum[start] + batchPoints, side='right')) - 1
        if end <= start:
            end = start + 1                     # one segment larger than the budget
        ranges.append((idLo + start, idLo + end))
        start = end
    return ranges


def iterSegmentPoints(seg, band, imgNullVal, tileSize=TILESIZE, maxSegId=None, batchPoints=None):
    """
    Every segment's points, batch by batch: yields (ids, offsets, pts) for consecutive id ranges,
    ascending from 1 to maxSegId (default: the largest label).  The points of ids[k] are
    pts[offsets[k]:offsets[k + 1]]; an id without points has an empty slice.  ``pts`` is a read-only
    numpy.recarray of SEGPOINT_DTYPE (fields x = column, y = row, val = band value as int64), so
    ``pt.x`` and ``pts.x`` both work.

    A point is a pixel whose label is not 0 and whose band value is not imgNullVal (None: every
    labelled pixel).  A segment's points come in the order in which the reference's
    accumulateSegSpatial appends them (tilingstats.py:1652-1699): the raster is visited in
    tileSize x tileSize tiles, tiles in row-major order, pixels row-major inside a tile.

    The GPU sorts the points once, then builds batch b + 1 into a second pinned host buffer while
    the caller works on batch b: a batch's points are overwritten once the generator advances past
    the next batch (copy what must outlive it).  Each batch holds at most ``batchPoints`` points (default POINTS_BATCH), except
    that a segment with more points than that comes in a batch of its own.
    """
    (seg, band) = _spatialArrays(seg, band)
    if maxSegId is None:
        maxSegId = int(seg.max()) if seg.size else 0
    maxSegId = int(maxSegId)
    if batchPoints is None:
        batchPoints = POINTS_BATCH
    if int(tileSize) < 1:
        raise PyShepSegStatsError("tileSize must be positive")
    nullV = numpy.iinfo(numpy.int64).min if imgNullVal is None else int(imgNullVal)
    dt = _lib.SHP_DTYPES[band.dtype]
    (nrows, ncols) = seg.shape
    c = _lib.Context()              # its own context: the sorted points live in its workspace between calls
    L = c._L
    devBufs = []
    hostBufs = []                   # (the context goes with the generator or with the last batch, later)

    def devAlloc(nbytes):
        p = ctypes.c_void_p()
        c.check(L.shp_dev_alloc(c.handle, nbytes, ctypes.byref(p)))
        devBufs.append(p)
        return p

    try:
        dseg = devAlloc(seg.nbytes)
        dband = devAlloc(band.nbytes)
        c.check(L.shp_dev_upload(c.handle, dseg, _lib.ptr(seg), seg.nbytes))
        c.check(L.shp_dev_upload(c.handle, dband, _lib.ptr(band), band.nbytes))
        counts = numpy.zeros(maxSegId + 1, dtype=numpy.uint32)
        c.check(L.shp_segpoints_count_dev(c.handle, dseg, dband, dt, nrows, ncols, maxSegId, nullV,
                                          _lib.ptr(counts)))
        batches = planPointBatches(counts, batchPoints)
        cum = numpy.concatenate([[0], numpy.cumsum(counts, dtype=numpy.int64)])
        cap = max([int(cum[hi] - cum[lo]) for (lo, hi) in batches] + [1])
        hostBufs = [_PinnedBuffer(c, cap * SEGPOINT_DTYPE.itemsize) for _k in range(min(2, len(batches)))]
        npts = ctypes.c_int64(0)
        c.check(L.shp_segpoints_build_dev(c.handle, dseg, dband, dt, nrows, ncols, maxSegId, nullV,
                                          int(tileSize), ctypes.byref(npts)))
        if npts.value != int(cum[-1]):
            raise PyShepSegStatsError("internal: %d points sorted, %d counted" % (npts.value, int(cum[-1])))

        def emit(lo, hi, offs, buf, n):
            c.check(L.shp_segpoints_emit(c.handle, lo, hi, _lib.ptr(offs), buf, cap, ctypes.byref(n)))
        yield from emitPointBatches(batches, hostBufs, emit)       # (closing this closes that: its thread ends first)
    finally:
        for p in devBufs:
            L.shp_dev_free(c.handle, p)


def emitPointBatches(batches, hostBufs, emit):
    """The double-buffered emission of iterSegmentPoints: batch b + 1 is emitted (in a worker thread) into one
    of the two pinned hostBufs while the caller works on batch b.  ``emit(lo, hi, offs, bufPtr, n)`` fills the
    points of ids [lo, hi) and their offsets (offs: hi - lo + 1 int64) and sets the ctypes int64 ``n`` to their
    number.  Yields (ids, offsets, pts) for the (lo, hi) ranges of ``batches``, in order."""
    def one(b):
        (lo, hi) = batches[b]
        offs = numpy.empty(hi - lo + 1, dtype=numpy.int64)
        n = ctypes.c_int64(0)
        emit(lo, hi, offs, hostBufs[b % 2].p, n)
        return (offs, n.value)

    with concurrent.futures.ThreadPoolExecutor(max_workers=1) as pool:
        nxt = pool.submit(one, 0) if batches else None
        for b in range(len(batches)):
            (offs, n) = nxt.result()
            nxt = pool.submit(one, b + 1) if b + 1 < len(batches) else None
            pts = hostBufs[b % 2].points(n)
            offs.flags.writeable = False
            (lo, hi) = batches[b]
            yield (numpy.arange(lo, hi, dtype=shepseg.SegIdType), offs, pts)
        # (leaving the block waits for an emission still running: its buffer is freed by its owner)


def convertPtsInto2DArray(pts, imgNullVal):
    """A segment's points (a recarray of SEGPOINT_DTYPE, or anything with x, y and val fields) as an
    int64 array over their bounding box: each point's value at (y - ymin, x - xmin), imgNullVal
    elsewhere (reference tilingstats.py:1744-1793)."""
    (x, y) = (numpy.asarray(pts.x, dtype=numpy.int64), numpy.asarray(pts.y, dtype=numpy.int64))
    (xmin, ymin) = (x.min(), y.min())
    tile = numpy.full((y.max() - ymin + 1, x.max() - xmin + 1), imgNullVal, dtype=numpy.int64)
    tile[y - ymin, x - xmin] = pts.val
    return tile


def convertPtsInto2DMaskArray(pts, imgNullVal):
    """As convertPtsInto2DArray, with uint8 1 at the segment's points and 0 elsewhere (reference
    tilingstats.py:1796-1844; imgNullVal is not used, as there)."""
    (x, y) = (numpy.asarray(pts.x, dtype=numpy.int64), numpy.asarray(pts.y, dtype=numpy.int64))
    (xmin, ymin) = (x.min(), y.min())
    tile = numpy.zeros((y.max() - ymin + 1, x.max() - xmin + 1), dtype=numpy.uint8)
    tile[y - ymin, x - xmin] = 1
    return tile


def runUserFunc(batches, numRows, userFunc, userParam, imgNullVal, numIntCols, numFloatCols,
                missingStatsValue=-9999):
    """The per-segment calls of calcStatsForCompletedSegsSpatial (reference tilingstats.py:1847-1932)
    over (ids, offsets, pts) batches as iterSegmentPoints yields them: for every id with points,
    intArr (int32, numIntCols) and floatArr (float64, numFloatCols) are filled with
    missingStatsValue, ``userFunc(pts, imgNullVal, intArr, floatArr, userParam)`` is called, and the
    arrays become the id's row of intcols (int64) and floatcols (float32).  Ids without points (all
    nodata, or no pixels at all) keep missingStatsValue; row 0 is zero.  Returns (intcols
    (numIntCols, numRows), floatcols (numFloatCols, numRows)).  An exception of userFunc propagates."""
    intcols = numpy.full((numIntCols, numRows), missingStatsValue, dtype=numpy.int64)
    floatcols = numpy.full((numFloatCols, numRows), missingStatsValue, dtype=numpy.float32)
    if numRows:
        intcols[:, 0] = 0
        floatcols[:, 0] = 0
    intArr = numpy.empty(numIntCols, dtype=numpy.int32)
    floatArr = numpy.empty(numFloatCols, dtype=numpy.float64)
    for (ids, offs, pts) in batches:
        for k in numpy.flatnonzero(offs[1:] != offs[:-1]):
            intArr.fill(missingStatsValue)
            floatArr.fill(missingStatsValue)
            userFunc(pts[offs[k]:offs[k + 1]], imgNullVal, intArr, floatArr, userParam)
            segId = ids[k]
            intcols[:, segId] = intArr
            floatcols[:, segId] = floatArr
    return intcols, floatcols


def calcPerSegmentSpatialStats(seg, band, colTypes, userFunc, userParam, imgNullVal,
                               missingStatsValue=-9999, maxSegId=None, tileSize=TILESIZE):
    """The compute step on arrays: colTypes = list of GFT_Integer / GFT_Real in column order.
    Returns (intcols int64 (nInt, maxSegId+1), floatcols float32 (nFloat, maxSegId+1)).  The
    built-in user functions run on the GPU; a user function (decorated with spatialUserFunc, or
    @jit / @njit) is called per segment with the points of iterSegmentPoints(seg, band, imgNullVal,
    tileSize) (see runUserFunc).  Any other userFunc is refused."""
    (seg, band) = _spatialArrays(seg, band)
    if maxSegId is None:
        maxSegId = int(seg.max()) if seg.size else 0
    nInt = sum(1 for t in colTypes if t == GFT_Integer)
    nFloat = sum(1 for t in colTypes if t == GFT_Real)
    if nInt + nFloat != len(colTypes):
        raise PyShepSegStatsError("column types must be GFT_Integer or GFT_Real")
    if not isinstance(userFunc, _BuiltinSpatialFunc):
        if not _isUserFunc(userFunc):
            raise PyShepSegStatsError(
                "userFunc must be one of the built-in user functions (userFuncMeanCoord, "
                "userFuncNumEdgePixels, userFuncVariogram), or a function decorated with "
                "tilingstats.spatialUserFunc (or @jit / @njit)")
        with contextlib.closing(iterSegmentPoints(seg, band, imgNullVal, tileSize, maxSegId)) as batches:
            return runUserFunc(batches, maxSegId + 1, userFunc, userParam, imgNullVal, nInt, nFloat,
                               missingStatsValue)
    params = numpy.zeros(6, dtype=numpy.float64)
    pv = numpy.atleast_1d(numpy.asarray(0 if userParam is None else userParam, dtype=numpy.float64))
    params[:min(len(pv), 6)] = pv[:6]
    intcols = numpy.zeros((max(nInt, 1), maxSegId + 1), dtype=numpy.int64)
    floatcols = numpy.zeros((max(nFloat, 1), maxSegId + 1), dtype=numpy.float32)
    c = _lib.ctx()
    c.check(c._L.shp_spatialstats(c.handle, _lib.ptr(seg), _lib.ptr(band), _lib.SHP_DTYPES[band.dtype],
                                  seg.shape[0], seg.shape[1], maxSegId, int(imgNullVal),
                                  userFunc.funcId, _lib.ptr(params), int(missingStatsValue), nInt,
                                  nFloat, _lib.ptr(intcols), _lib.ptr(floatcols)))
    return intcols[:nInt], floatcols[:nFloat]


def variogramRecomputed():
    """The (segment, bin) pairs the calling thread's last built-in variogram recomputed in the reference's
    float64 order, because a squared difference or a bin's integer sum reached 2^53 (wide 32-bit imagery, or very
    large segments): 0 when the integer sums were the reference's sums already."""
    c = _lib.ctx()
    n = ctypes.c_int64(0)
    c.check(c._L.shp_spatial_vario_redo_count(c.handle, ctypes.byref(n)))
    return int(n.value)


def calcPerSegmentSpatialStatsTiled(imgfile, imgbandnum, segfile, colNamesAndTypes, userFunc,
        userParam=None, missingStatsValue=-9999, imgNullVal=None, tileSize=TILESIZE):
    """
    Spatial per-segment statistics (reference tilingstats.py:1262-1390).  ``userFunc`` is a
    callable ``userFunc(pts, imgNullVal, intArr, floatArr, userParam)`` decorated with
    ``spatialUserFunc`` (where the reference requires @jit / @njit, which is accepted too; an
    undecorated callable is refused, as in the reference), called once for every
    segment with at least one non-nodata pixel: ``pts`` holds those pixels as points with fields
    x, y (column and row in the whole image) and val, in the reference's order (tileSize x tileSize
    tiles row-major, pixels row-major inside a tile); ``intArr`` (int32) and ``floatArr``
    (float64), one entry per Integer / Real column in the order of ``colNamesAndTypes``, arrive
    filled with missingStatsValue and are stored as int64 / float32 columns.  Unlike the reference,
    which calls the function as segments complete, segments are called in ascending id order.
    ``convertPtsInto2DArray`` / ``convertPtsInto2DMaskArray`` give a segment's bounding-box tile.

    This module's ``userFuncMeanCoord`` (userParam = the six geotransform numbers; two Real
    columns), ``userFuncNumEdgePixels`` (userParam = fourConnected; one Integer column) and
    ``userFuncVariogram`` (userParam = maxDist; maxDist Real columns) stand for the reference's
    examples and run as reductions on the GPU (their mean coordinates do not depend on tileSize).
    ``colNamesAndTypes`` is the reference's list of (name, GFT_Integer | GFT_Real).
    ``imgNullVal`` stands for the image band's nodata value, which must be set (the reference
    raises the same error, tilingstats.py:1325-1333).  Segments whose pixels are all nodata, and
    ids without pixels, get missingStatsValue; row 0 is zero.  Returns a TiledStatsResult whose
    ``columns`` maps column name -> array (one row per id).
    """
    timings = Timers()
    if imgNullVal is None:
        raise PyShepSegStatsError("NoData value must be set on imgfile")
    if len(colNamesAndTypes) == 0:
        raise PyShepSegStatsError("Must specify one or more columns")
    with timings.interval('reading'):
        seg = _loadArray(segfile)
        img = _loadArray(imgfile, imgbandnum)
        if seg is None or img is None:
            raise PyShepSegStatsError("GDAL is not available here: pass numpy arrays or .npy paths")
    with timings.interval('accumulation'):
        (intcols, floatcols) = calcPerSegmentSpatialStats(
            seg, img, [t for (_n, t) in colNamesAndTypes], userFunc, userParam, imgNullVal,
            missingStatsValue, tileSize=tileSize)
    cols = {}
    ni = nf = 0
    for (name, t) in colNamesAndTypes:
        if t == GFT_Integer:
            cols[name] = intcols[ni]
            ni += 1
        else:
            cols[name] = floatcols[nf]
            nf += 1
    rtn = TiledStatsResult()
    rtn.timings = timings
    rtn.columns = cols
    return rtn
