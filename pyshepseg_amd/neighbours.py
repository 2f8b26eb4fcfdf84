"""Per-segment neighbour lists and border lengths of a label raster.

The reference stops at statistics that describe a segment by itself; an object-based workflow next asks
which segments touch which, and along how much border (neighbour context for a classification, "relative
border to", merge candidates, colouring the segments like a map).  ``findSegmentNeighbours`` answers that
from the label raster alone, on the GPU (csrc/neighbours.h), as a CSR table over the segment ids.

Definition, all integers: two pixels are adjacent when one is the E or S neighbour of the other, and with
``fourConnected=False`` the SE and SW neighbour as well.  Every adjacent pixel pair with labels ``a != b``,
both non-zero, adds 1 to the border length of ``(a, b)`` and of ``(b, a)``.  Label 0 is no segment: it has
no neighbours and is nobody's neighbour.  Ids without pixels have empty rows.

There is no CPU fallback: without a GPU the call fails as every entry point of this package does.
"""
import ctypes
import time

import numpy

from . import _lib
from . import shepseg
from . import tiling
from . import tilingstats


class PyShepSegNeighboursError(Exception):
    pass


class SegmentNeighbours(object):
    """The CSR table of findSegmentNeighbours.

    ``offsets``: int64, ``maxSegId + 2`` row boundaries (``offsets[0] == offsets[1] == 0``);
    ``neighbours``: uint32 neighbour ids, ascending within a row; ``borderLengths``: int64, the pixel pairs
    shared with that neighbour.  ``pairsSeen``: differing pixel pairs met; ``recordsSorted``: (pair, count)
    records the patches handed to the global sort; ``blocksRerun``: row blocks whose records did not fit the
    buffer and that ran a second time.  ``timings``: seconds per step; ``deviceMs``: GPU time of the kernels."""
    def __init__(self, offsets, neighbours, borderLengths, maxSegId, fourConnected, pairsSeen=0, recordsSorted=0,
                 timings=None, deviceMs=None, blocksRerun=0):
        self.offsets = offsets
        self.neighbours = neighbours
        self.borderLengths = borderLengths
        self.maxSegId = maxSegId
        self.fourConnected = fourConnected
        self.pairsSeen = pairsSeen
        self.recordsSorted = recordsSorted
        self.blocksRerun = blocksRerun
        self.timings = timings if timings is not None else {}
        self.deviceMs = deviceMs

    def neighboursOf(self, segId):
        """(ids, lengths) of one segment: views of ``neighbours`` and ``borderLengths``"""
        segId = int(segId)
        if segId < 0 or segId > self.maxSegId:
            raise PyShepSegNeighboursError("segment id {} is outside 0..{}".format(segId, self.maxSegId))
        (a, b) = (int(self.offsets[segId]), int(self.offsets[segId + 1]))
        return (self.neighbours[a:b], self.borderLengths[a:b])

    @property
    def columns(self):
        """{'numNeighbours', 'borderLength'}: int64 per id, the row's length and the row's sum, as the
        statistics' column dictionaries hold them"""
        num = numpy.diff(self.offsets)
        total = numpy.zeros(len(num), dtype=numpy.int64)
        rows = numpy.flatnonzero(num)
        if len(rows):
            total[rows] = numpy.add.reduceat(self.borderLengths, self.offsets[rows])
        return {'numNeighbours': num, 'borderLength': total}


def _checkArgs(segfile, maxSegId):
    """(host labels or None, device labels or None, rows, columns, maxSegId or None): everything that can be
    refused before the GPU is touched"""
    if maxSegId is not None:
        if int(maxSegId) != maxSegId or maxSegId < 0:
            raise PyShepSegNeighboursError("maxSegId must be a non-negative integer (got {})".format(maxSegId))
        maxSegId = int(maxSegId)
        if maxSegId >= 0xFFFFFFFE:
            raise PyShepSegNeighboursError("maxSegId {} is too large".format(maxSegId))
    if getattr(segfile, 'outDev', None):
        (devSeg, nrows, ncols, _nbytes) = segfile.outDev
        return (None, devSeg, nrows, ncols, maxSegId)
    seg = tilingstats._loadArray(getattr(segfile, 'segimg', None) if isinstance(
        segfile, tiling.TiledSegmentationResult) else segfile)
    if seg is None or seg.ndim != 2 or seg.dtype != shepseg.SegIdType:
        raise PyShepSegNeighboursError("segfile must be a 2-D uint32 array, a .npy path of one, or a "
                                       "segmentation result kept on the device")
    return (seg, None, seg.shape[0], seg.shape[1], maxSegId)


def findSegmentNeighbours(segfile, fourConnected=True, maxSegId=None, chunkPixels=None):
    """
    Which segments touch which, and along how many pixel pairs: a SegmentNeighbours.

    ``segfile`` is a 2-D uint32 array, a ``.npy`` path (memory-mapped: the raster may be larger than HBM), a
    TiledSegmentationResult (its ``segimg``), or the result of
    ``doTiledShepherdSegmentation(..., outfile=tiling._KEEP_ON_DEVICE)`` whose labels are in HBM and are read
    in place.  ``maxSegId`` is the table's last row; None takes the largest label, found on the GPU.  A label
    above a given ``maxSegId`` raises PyShepSegNeighboursError with the largest such label.

    The labels stream through the GPU in row blocks of ``chunkPixels`` pixels (default
    tilingstats.STATS_CHUNK_PIXELS), each with the row that follows it; the table does not depend on the blocks.
    """
    (seg, devSeg, nrows, ncols, maxSegId) = _checkArgs(segfile, maxSegId)
    if chunkPixels is None:
        chunkPixels = tilingstats.STATS_CHUNK_PIXELS
    rowsPerChunk = max(1, min(max(nrows, 1), int(chunkPixels) // max(ncols, 1)))
    t0 = time.perf_counter()
    c = _lib.ctx()
    L = c._L
    src = tilingstats._ChunkSource(c, seg, [], devSeg=devSeg, devPlanes=[], bandDtype=numpy.uint8, shape=(nrows, ncols))
    timings = {}
    try:
        c.check(L.shp_nbr_begin(c.handle, -1 if maxSegId is None else maxSegId, int(bool(fourConnected))))
        if ncols > 0:
            for y0 in range(0, nrows, rowsPerChunk):
                y1 = min(nrows, y0 + rowsPerChunk)
                more = y1 < nrows
                (dseg, _planes) = src.chunk(y0, y1 + (1 if more else 0))
                c.check(L.shp_nbr_accumulate_dev(c.handle, dseg, y1 - y0, ncols, int(more)))
        timings['accumulate'] = time.perf_counter() - t0
        t1 = time.perf_counter()
        (S, nent, bad) = (ctypes.c_uint32(0), ctypes.c_int64(0), ctypes.c_uint32(0))
        counters = numpy.zeros(3, dtype=numpy.int64)
        ms = ctypes.c_double(0)
        c.check(L.shp_nbr_finish(c.handle, ctypes.byref(S), ctypes.byref(nent), ctypes.byref(bad), _lib.ptr(counters),
                                 ctypes.byref(ms)))
        if bad.value:
            raise PyShepSegNeighboursError("segment id {} is above maxSegId {}".format(bad.value, S.value))
        timings['finish'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        offsets = numpy.empty(S.value + 2, dtype=numpy.int64)
        nbrs = numpy.empty(nent.value, dtype=numpy.uint32)
        lens = numpy.empty(nent.value, dtype=numpy.int64)
        c.check(L.shp_nbr_download(c.handle, _lib.ptr(offsets), _lib.ptr(nbrs), _lib.ptr(lens)))
        timings['download'] = time.perf_counter() - t1
    finally:
        src.close()
    timings['total'] = time.perf_counter() - t0
    return SegmentNeighbours(offsets, nbrs, lens, S.value, bool(fourConnected), pairsSeen=int(counters[0]),
                             recordsSorted=int(counters[1]), timings=timings, deviceMs=ms.value,
                             blocksRerun=int(counters[2]))
