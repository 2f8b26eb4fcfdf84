"""The label raster under the per-segment calls on one GPU: what ``segfile`` may be, the row blocks it streams through
the device in, its largest label, and the loop that turns every block of labels into a block of output.  The entry
points of neighbours, shapes, outlines, depths and utils.renderColourTable start here, each with a short ``_checkArgs``
that lists its own checks in its own order and passes its exception class as ``Err``: every refusal is raised as that.
The statistics, whose blocks carry image planes as well, keep tilingstats._ChunkSource.  No caller is imported at load.
"""
import collections
import ctypes

import numpy

from . import _lib
from . import shepseg
from . import tiling
from . import tilingstats

# host labels or None, device labels (an address) or None, rows, columns, maxSegId or None
Labels = collections.namedtuple('Labels', ('seg', 'devSeg', 'nrows', 'ncols', 'maxSegId'))


def resolve(segfile, maxSegId, Err, merged=False, hint=False):
    """The Labels of ``segfile``: a 2-D uint32 array, a ``.npy`` path of one (memory-mapped), a TiledSegmentationResult
    (its ``segimg``) or anything with ``outDev`` (labels in HBM, read in place); with ``merged`` also a MergedSegments:
    its ``outDev`` if it has one, else its ``segimg``.  ``hint``: a ``maxSegId`` of None is taken from a result object
    that carries one.  Nothing here touches the GPU."""
    if hint and maxSegId is None and getattr(segfile, 'maxSegId', None) is not None and not isinstance(segfile, numpy.ndarray):
        maxSegId = int(segfile.maxSegId)
    if merged and not getattr(segfile, 'outDev', None):
        from . import neighbours
        if isinstance(segfile, neighbours.MergedSegments):
            if segfile.segimg is None:
                raise Err("the MergedSegments holds no recoded raster: neither outDev nor segimg")
            segfile = segfile.segimg
    if maxSegId is not None:
        if int(maxSegId) != maxSegId or maxSegId < 0:
            raise Err("maxSegId must be a non-negative integer (got {})".format(maxSegId))
        maxSegId = int(maxSegId)
        if maxSegId >= 0xFFFFFFFE:
            raise Err("maxSegId {} is too large".format(maxSegId))
    if getattr(segfile, 'outDev', None):
        (devSeg, nrows, ncols, _nbytes) = segfile.outDev
        return Labels(None, devSeg, nrows, ncols, maxSegId)
    seg = tilingstats._loadArray(getattr(segfile, 'segimg', None) if isinstance(
        segfile, tiling.TiledSegmentationResult) else segfile)
    if seg is None or seg.ndim != 2 or seg.dtype != shepseg.SegIdType:
        raise Err("segfile must be a 2-D uint32 array, a .npy path of one, or a segmentation result kept on the device")
    return Labels(seg, None, seg.shape[0], seg.shape[1], maxSegId)


def number(value, name, Err):
    if isinstance(value, (bool, numpy.bool_)) or not isinstance(value, (int, float, numpy.integer, numpy.floating)):
        raise Err("{} must be a number (got {!r})".format(name, value))
    return float(value)


def checkOrigin(origin, nrows, ncols, Err):
    """(row0, col0) as integers: the coordinates of the first pixel of a raster of nrows x ncols, all below 2^32"""
    try:
        (row0, col0) = origin
    except (TypeError, ValueError):
        raise Err("origin must be (row0, col0) (got {!r})".format(origin))
    for v in (row0, col0):
        if isinstance(v, (bool, numpy.bool_)) or not isinstance(v, (int, numpy.integer)) or v < 0:
            raise Err("origin must be two non-negative integers (got {!r})".format(origin))
    (row0, col0) = (int(row0), int(col0))
    if row0 + nrows > 2 ** 32 or col0 + ncols > 2 ** 32:
        raise Err("origin {} puts a {} x {} raster past coordinate 2^32".format((row0, col0), nrows, ncols))
    return (row0, col0)


def checkChunkPixels(chunkPixels, Err):
    """the pixels of a streamed block as a positive integer; None: tilingstats.STATS_CHUNK_PIXELS"""
    chunkPixels = tilingstats.STATS_CHUNK_PIXELS if chunkPixels is None else chunkPixels
    if isinstance(chunkPixels, (bool, numpy.bool_)) or not isinstance(chunkPixels, (int, numpy.integer)) or chunkPixels < 1:
        raise Err("chunkPixels must be a positive integer (got {!r})".format(chunkPixels))
    return int(chunkPixels)


def rowBlocks(nrows, ncols, chunkPixels, above=False, below=False):
    """The row blocks [y0, y1) a raster streams in, whole rows of about ``chunkPixels`` pixels (None:
    tilingstats.STATS_CHUNK_PIXELS; less than a row: one row), as a list of (y0, y1, hasAbove, hasBelow): whether the
    block comes with the row above and the row below it, as ``above`` and ``below`` ask wherever the raster has one."""
    pixels = tilingstats.STATS_CHUNK_PIXELS if chunkPixels is None else int(chunkPixels)
    step = max(1, min(max(nrows, 1), pixels // max(ncols, 1)))
    return [(y0, min(nrows, y0 + step), bool(above) and y0 > 0, bool(below) and y0 + step < nrows)
            for y0 in range(0, nrows if ncols else 0, step)]


class LabelSource(tilingstats._ChunkSource):
    """The labels of a Labels record as device pointers on context ``c``, a _ChunkSource without planes: resident labels
    are addressed in place, a host array or memory map goes up into a device buffer that is reused from block to block.
    A source is read either whole or in blocks.  Leaving the ``with`` frees the buffers."""
    def __init__(self, c, labels):
        tilingstats._ChunkSource.__init__(self, c, labels.seg, [], devSeg=labels.devSeg, devPlanes=[], shape=labels[2:4])
        self._whole = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def blocks(self, chunkPixels=None, above=False, below=False):
        """(y0, y1, dseg, hasAbove, hasBelow) for every block of rowBlocks, one after the other: ``dseg`` points at the
        first row handed over, row y0 - hasAbove, and holds until the next block is asked for"""
        plan = rowBlocks(self.nrows, self.ncols, chunkPixels, above, below)
        return ((y0, y1, self.chunk(y0 - hasAbove, y1 + hasBelow)[0], hasAbove, hasBelow)
                for (y0, y1, hasAbove, hasBelow) in plan)

    def whole(self):
        """the whole raster in HBM, uploaded by the first call; None for a raster without pixels"""
        if self._whole is None and self.nrows * self.ncols:
            self._whole = self.chunk(0, self.nrows)[0]
        return self._whole

    def labelMax(self, Err, chunkPixels=None):
        """(largest label, device ms of finding it): one reduction over whole() when the labels are resident or
        ``chunkPixels`` is None, otherwise one per block of blocks(chunkPixels), a host raster going up for it"""
        if self.devSeg is not None or chunkPixels is None:
            parts = [(self.nrows, self.whole())] if self.nrows * self.ncols else []
        else:
            parts = ((y1 - y0, dseg) for (y0, y1, dseg, _above, _below) in self.blocks(chunkPixels))
        (top, deviceMs, m, ms) = (0, 0.0, ctypes.c_uint32(0), ctypes.c_double(0))
        for (rows, dseg) in parts:
            self.c.check(self.c._L.shp_shape_label_max_dev(self.c.handle, dseg, rows * self.ncols, ctypes.byref(m), ctypes.byref(ms)))
            (top, deviceMs) = (max(top, m.value), deviceMs + ms.value)
        if top >= 0xFFFFFFFE:
            raise Err("label {} is too large".format(top))
        return (top, deviceMs)

    def alignedScratch(self, dseg, nbytes):
        """``nbytes`` of device scratch for the output of the block at ``dseg``, reused from block to block.  It starts
        at the labels' offset from a 16-byte boundary: the kernel then stores whole vectors"""
        return ctypes.c_void_p(self.scratch(0, nbytes + 16).value + (dseg.value & 15))


def mapBlocks(src, chunkPixels, call, dtype, pixelShape=(), outfile=None, devOut=None):
    """Every block of ``src.blocks(chunkPixels)`` through ``call(y0, y1, dseg, dout)``, which has the library write the
    block's output, (y1 - y0) * ncols pixels of ``pixelShape`` values of ``dtype``, at ``dout``.  The output goes into the
    ``.npy`` file ``outfile``, rows at a time; or stays where it was written, in the caller's device raster ``devOut`` (a
    c_void_p); or comes back as a host array (None is returned otherwise).  ``call`` returns whether the host wants the
    block: one it returns False for is neither downloaded nor written."""
    (c, nrows, ncols) = (src.c, src.nrows, src.ncols)
    pixelBytes = numpy.dtype(dtype).itemsize * int(numpy.prod(pixelShape, dtype=numpy.int64))
    plan = rowBlocks(nrows, ncols, chunkPixels)
    (writer, out) = (None, None)
    try:
        if outfile is not None:
            writer = tiling._NpyRowWriter(outfile, nrows, ncols, dtype=dtype, pixelShape=pixelShape)
            block = numpy.empty((plan[0][1] if plan else 0, ncols) + pixelShape, dtype=dtype)
        elif devOut is None:
            out = numpy.empty((nrows, ncols) + pixelShape, dtype=dtype)
        for (y0, y1, dseg, _above, _below) in src.blocks(chunkPixels):
            nbytes = (y1 - y0) * ncols * pixelBytes
            dout = (src.alignedScratch(dseg, nbytes) if devOut is None else
                    ctypes.c_void_p(devOut.value + pixelBytes * y0 * ncols))
            if call(y0, y1, dseg, dout) and devOut is None:
                dest = block[:y1 - y0] if writer is not None else out[y0:y1]
                c.check(c._L.shp_dev_download(c.handle, _lib.ptr(dest), dout, nbytes))
                if writer is not None:
                    writer.writeRows(y0, y1, dest)
    finally:
        if writer is not None:
            writer.close()
    return out
