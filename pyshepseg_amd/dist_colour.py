"""Colour tables from per-segment columns and the RGBA rendering on the row-sharded multi-rank output
(deviceColourTable, deviceRender; csrc/colour.h)."""
import collections.abc
import ctypes
import os

import numpy

from . import _lib
from . import distdev
from . import tiling
from .distdev import (idRange, _addr, _stepOnAllRanks, checkNpyOutfile, _mosaicPieces, overviewTable,
                      overviewHoles)


RENDER_BLOCK_PIXELS = 1 << 24      # pixels per lookup / download block: 64 MB each way, several blocks per rank
RENDER_GROUP_BLOCKS = 4            # blocks per pinned staging buffer (and per write into the file)
_SEL_PASSES = 8                    # csrc/colour.h: SEL_PASSES, SEL_HIST_WORDS
_SEL_HIST_WORDS = 512
_COL_BAD = {1: "column holds a NaN or an infinity",
            2: "integer column holds a magnitude of 2^53 or more: not exact in float64"}


def colourShares(n, world):
    """The rows [lo, hi) of a column of n rows that each rank stretches: idRange of the ids 0..n-1, the share the
    statistics reduce by.  Consecutive, in rank order, empty where n < world."""
    return [idRange(r, world, n - 1) for r in range(world)]


def _colourShareOf(col, lo, hi):
    """rows [lo, hi) of a column as the library takes them (utils._stretchColumn): (contiguous float64 / float32 /
    int64 array, column type code)"""
    from . import utils
    part = col[lo:hi]
    if col.dtype.kind in 'iub':
        if col.dtype == numpy.uint64:
            # (2^63 and more does not fit int64: the largest int64 stands in, and is flagged on the device like any
            #  magnitude of 2^53 or more)
            part = numpy.minimum(part, numpy.uint64(numpy.iinfo(numpy.int64).max))
        part = part.astype(numpy.int64, copy=False)
    elif col.dtype not in utils._COLTYPE:
        part = part.astype(numpy.float64)
    part = numpy.ascontiguousarray(part)
    return part, utils._COLTYPE[part.dtype]


def deviceColourTable(c, comm, cols, info=None):
    """The device path of writeColorTableFromRatColumnsDistributed for ONE rank: ``cols`` = the red, green and blue
    source columns (1-D arrays with one row per segment id, the same on every rank), context ``c``; comm:
    allgather_obj, allgather_dev, allreduce_dev_i64.  Rank r uploads rows colourShares(n, world)[r] only.  Per
    column: shp_dcolour_begin -> eight times (shp_dcolour_hist over the share, one all-reduce of the digit
    histograms, shp_dcolour_pick: the same digits on every rank) -> shp_dcolour_finish: numpy's 5th and 95th
    percentile of the WHOLE column -> shp_dcolour_stretch_dev on the share -> one all-gather of the byte shares
    (padded to the largest), compacted into the whole byte column.  Then Alpha = 255 and shp_colour_pack_dev: the
    packed table never leaves the device.  Lengths and types are all-gathered before any device work, the
    non-finite / wide-integer flags ride in the first histogram block: every error is raised on every rank, as
    utils.PyShepSegUtilsError.
    Returns (columns {Red, Green, Blue, Alpha: uint8 (n,)}, [(lo, hi)] * 3 as numpy.float64, device ms, d_table
    (c_void_p: n packed words, the caller frees it with tiling._devRelease(c, d_table, 4 n)), n).  ``info`` (a dict,
    optional): 'rows' (this rank's share), 'exchange_bytes' (of all ranks, without padding), 'deviceMs'."""
    from . import utils
    Err = utils.PyShepSegUtilsError
    L = c._L
    err = None
    key = None
    try:
        cols = [numpy.asarray(col) for col in cols]
        if len(cols) != 3:
            raise Err("three columns (red, green, blue) are needed")
        for col in cols:
            if col.ndim != 1 or col.size == 0:
                raise Err("a column must be a non-empty 1-D array")
            if col.dtype.kind not in 'iubf':
                raise Err("a column of type %s cannot be stretched" % col.dtype)
        if len(set(len(col) for col in cols)) != 1:
            raise Err("the three columns differ in length")
        if len(cols[0]) >= 1 << 32:
            raise Err("a column of %d rows: 2^32 or more are not supported" % len(cols[0]))
        key = (len(cols[0]), tuple(_colourShareOf(col, 0, 0)[1] for col in cols))
    except Err as e:
        err = str(e)
    got = comm.allgather_obj((err, key))                                            # control data
    distdev.raiseFirst(Err, [g[0] for g in got])
    if len(set(g[1][0] for g in got)) != 1:
        raise Err("the columns differ in length between the ranks (%s rows)" % ', '.join(str(g[1][0]) for g in got))
    if len(set(g[1][1] for g in got)) != 1:
        raise Err("the columns differ in type between the ranks")
    n = key[0]
    shares = colourShares(n, comm.world)
    (lo, hi) = shares[comm.rank]
    m = hi - lo
    slot = (max(b - a for (a, b) in shares) + 15) // 16 * 16
    pitch = (n + 15) // 16 * 16
    stretch = []
    deviceMs = 0.0
    with distdev.Scratch(c) as s:
        d_table = s.alloc(n * 4)
        d_bytes = s.alloc(4 * pitch)
        d_send = s.alloc(slot) if comm.world > 1 else None
        d_all = s.alloc(comm.world * slot) if comm.world > 1 else None
        for (k, col) in enumerate(cols):
            (part, ctype) = _colourShareOf(col, lo, hi)
            d_block = ctypes.c_void_p()
            c.check(L.shp_dcolour_begin(c.handle, _lib.ptr(part) if m else None, ctype, m, n, ctypes.byref(d_block)))
            for p in range(_SEL_PASSES):
                c.check(L.shp_dcolour_hist(c.handle, p))
                if comm.world > 1:
                    comm.allreduce_dev_i64(d_block.value, _SEL_HIST_WORDS + (1 if p == 0 else 0))
                c.check(L.shp_dcolour_pick(c.handle, p))
            lohi = numpy.zeros(2, dtype=numpy.float64)
            bad = ctypes.c_int(0)
            c.check(L.shp_dcolour_finish(c.handle, _lib.ptr(lohi), ctypes.byref(bad)))
            if bad.value:           # (the summed flags: the same on every rank)
                raise Err(_COL_BAD[2] if bad.value & 2 else _COL_BAD[1])
            stretch.append((numpy.float64(lohi[0]), numpy.float64(lohi[1])))
            ms = ctypes.c_double(0)
            d_col = ctypes.c_void_p(d_bytes.value + k * pitch)
            if comm.world == 1:
                c.check(L.shp_dcolour_stretch_dev(c.handle, d_col, ctypes.byref(ms)))
            else:
                c.check(L.shp_dcolour_stretch_dev(c.handle, d_send, ctypes.byref(ms)))
                comm.allgather_dev(d_send.value, d_all.value, slot)
                for (r, (a, b)) in enumerate(shares):
                    if b > a:
                        c.check(L.shp_dev_copy(c.handle, ctypes.c_void_p(d_col.value + a),
                                               ctypes.c_void_p(d_all.value + r * slot), b - a))
            deviceMs += ms.value
        d_alpha = ctypes.c_void_p(d_bytes.value + 3 * pitch)
        c.check(L.shp_dev_memset(c.handle, d_alpha, 255, pitch))
        c.check(L.shp_colour_pack_dev(c.handle, d_bytes, ctypes.c_void_p(d_bytes.value + pitch),
                                      ctypes.c_void_p(d_bytes.value + 2 * pitch), d_alpha, n, d_table))
        host = numpy.empty((3, pitch), dtype=numpy.uint8)
        c.check(L.shp_dev_download(c.handle, _lib.ptr(host), d_bytes, host.nbytes))
        s.keep(d_table)             # (the caller's from here on)
    columns = {name: host[k, :n].copy() for (k, name) in enumerate(utils.COLOUR_NAMES[:3])}
    columns['Alpha'] = numpy.full(n, 255, dtype=numpy.uint8)
    if info is not None:
        blocks = _SEL_PASSES * _SEL_HIST_WORDS + 1
        info.update(rows=(lo, hi), deviceMs=deviceMs,
                    exchange_bytes=(3 * (blocks * 8 * comm.world + n)) if comm.world > 1 else 0)
    return columns, stretch, deviceMs, d_table, n


def writeColorTableFromRatColumnsDistributed(engine, comm, columns, redColName, greenColName, blueColName, info=None):
    """utils.writeColorTableFromRatColumns over the ranks of a multi-rank run: every rank calls it with the same
    ``columns`` -- a mapping of column name to a 1-D array with one row per segment id, e.g.
    statsColumnsByName(bandSelections, *calcPerSegmentStatsDistributedBands(...)) -- and gets the same
    utils.ColourTableResult: Red, Green, Blue and ``stretch`` bit-identical to the one-GPU function on the whole
    columns (numpy's bytes and percentiles) at every world size, Alpha 255 everywhere, row 0 taking part in the
    percentiles.  The work is shared by id (deviceColourTable): a rank uploads, selects in and stretches only its
    rows colourShares(n, world)[rank].  The packed table stays on the engine (``engine.colourTable``) for
    renderColourTableDistributed, until release() / releaseOutput().  A transport that is not on the device goes
    through comm.HostStagedDev.

    ``info`` (a dict, optional) receives 'rows', 'exchange_bytes' and 'deviceMs'.  Errors are
    utils.PyShepSegUtilsError, raised on every rank: a name that is not in ``columns``, columns of different
    length or a length that differs between the ranks, a NaN or an infinity or an integer of magnitude 2^53 or
    more in any rank's share, an engine without the device methods."""
    from . import utils
    Err = utils.PyShepSegUtilsError
    names = (redColName, greenColName, blueColName)
    err = None
    table = getattr(columns, 'columns', columns)
    if not hasattr(engine, 'colourTableOnDevice'):
        err = "writeColorTableFromRatColumnsDistributed needs a device engine (HipEngine)"
    elif not isinstance(table, collections.abc.Mapping):
        err = "columns must be a mapping of column name to array"
    else:
        for name in names:
            if name not in table:
                err = "column '{}' is not in the table".format(name)
                break
    distdev.raiseFirst(Err, comm.allgather_obj(err))
    dcomm = distdev.deviceComm(comm, engine.c)
    (cols, stretch, deviceMs) = engine.colourTableOnDevice(dcomm, [table[name] for name in names], info=info)
    return utils.ColourTableResult(cols, stretch, deviceMs)


class _NpyRgbaPatchWriter(tiling._NpyRowWriter):
    """_NpyPatchWriter for an existing (nRows, nCols, 4) uint8 .npy file (made by _NpyRowWriter with dtype uint8
    and pixelShape (4,)): opened for pwrite by any rank."""
    def __init__(self, path, nrows, ncols):
        with open(path, 'rb') as f:
            version = numpy.lib.format.read_magic(f)
            (shape, fortran, dtype) = numpy.lib.format._read_array_header(f, version)
            self.offset = f.tell()
        if shape != (nrows, ncols, 4) or fortran or dtype != numpy.dtype(numpy.uint8):
            raise tiling.PyShepSegTilingError("%s holds %s %s, not (%d, %d, 4) uint8" % (path, shape, dtype, nrows, ncols))
        (self.nrows, self.ncols, self.pixelBytes) = (nrows, ncols, 4)
        self.fd = os.open(path, os.O_WRONLY)

    def writeRect(self, y0, x0, v):
        """v (h x w x 4) at rows [y0, y0 + h), columns [x0, x0 + w): whole rows in one pwrite, else row by row"""
        (h, w) = v.shape[:2]
        if v.shape[2:] != (4,) or v.dtype != numpy.uint8:
            raise tiling.PyShepSegTilingError("an RGBA rectangle is (h, w, 4) uint8, not %s %s" % (v.shape, v.dtype))
        if y0 < 0 or x0 < 0 or y0 + h > self.nrows or x0 + w > self.ncols:
            raise tiling.PyShepSegTilingError("rectangle (%d, %d) + (%d, %d) leaves the (%d, %d) raster"
                                              % (y0, x0, h, w, self.nrows, self.ncols))
        if x0 == 0 and w == self.ncols:
            return self.writeRows(y0, y0 + h, v)
        for r in range(h):
            mv = memoryview(numpy.ascontiguousarray(v[r])).cast('B')
            pos = self.offset + ((y0 + r) * self.ncols + x0) * 4
            done = 0
            while done < len(mv):
                done += os.pwrite(self.fd, mv[done:], pos + done)


def deviceRender(c, comm, d_seg, nRows, nCols, d_table, nTable, rects=None, npacked=0, sink=None, blockPixels=None,
                 info=None):
    """The device path of renderColourTableDistributed for ONE rank: nRows x nCols labels (uint32) at d_seg in the
    HBM of context ``c`` (a rank without rows: nRows 0, d_seg None), painted through the packed table of nTable
    words at d_table; comm: allgather_obj.  shp_colour_render_rows_dev paints blocks of ``blockPixels`` pixels
    (default RENDER_BLOCK_PIXELS, whole rows) and downloads a block while the next is looked up, RENDER_GROUP_BLOCKS
    blocks per call into one pinned buffer; each group is handed to ``sink(y0, y1, rows)`` -- rows [y0, y1) of
    the held block as a (y1 - y0, nCols, 4) uint8 view that is valid during the call only -- or, without a sink,
    collected.  ``rects`` (int64 (k, 6), overviewTable's, ``npacked`` pixels): their colours, one launch
    (shp_colour_overview_rects_dev) and one download.  What failed on a rank, and the smallest label without a row
    in the table, are all-gathered: every rank raises the same utils.PyShepSegUtilsError.
    Returns (rows (nRows, nCols, 4) uint8 or None with a sink, colours (npacked, 4) uint8 or None).  ``info`` (a
    dict, optional): 'lookupMs', 'downloadMs' (summed device times of the blocks), 'renderMs' (wall time of the
    render calls: below their sum when the overlap pays), 'blocks'."""
    from . import utils
    Err = utils.PyShepSegUtilsError
    L = c._L
    (nRows, nCols, nTable) = (int(nRows), int(nCols), int(nTable))
    d_seg = _addr(d_seg)
    blockPixels = RENDER_BLOCK_PIXELS if blockPixels is None else int(blockPixels)
    rowsPerBlock = max(1, min(max(nRows, 1), min(blockPixels, 0x7fffffff) // max(nCols, 1)))
    rowsPerGroup = rowsPerBlock * RENDER_GROUP_BLOCKS
    out = None
    packed = None
    err = None
    missing = None
    times = [0.0, 0.0, 0.0]
    pin = None
    d_packed = None
    try:
        if sink is None:
            out = numpy.empty((nRows, nCols, 4), dtype=numpy.uint8)
        if nRows * nCols:
            pin = tiling._pinnedGet(c, min(nRows, rowsPerGroup) * nCols * 4)
        bad = (ctypes.c_uint32 * 2)()
        ms = (ctypes.c_double * 3)()
        for y0 in range(0, nRows if nCols else 0, rowsPerGroup):
            y1 = min(nRows, y0 + rowsPerGroup)
            c.check(L.shp_colour_render_rows_dev(c.handle, ctypes.c_void_p(d_seg + y0 * nCols * 4), (y1 - y0) * nCols,
                                                 rowsPerBlock * nCols, ctypes.c_void_p(_addr(d_table)), nTable,
                                                 ctypes.c_void_p(pin.ptr), bad, ms))
            for k in range(3):
                times[k] += ms[k]
            if bad[0]:
                missing = int(bad[1])
                break
            rows = pin.view(numpy.uint8, (y1 - y0, nCols, 4))
            if sink is not None:
                sink(y0, y1, rows)
            else:
                out[y0:y1] = rows
        if rects is not None and npacked and missing is None:
            rects = numpy.ascontiguousarray(rects, dtype=numpy.int64)
            d_packed = tiling._devAlloc(c, npacked * 4)
            c.check(L.shp_colour_overview_rects_dev(c.handle, ctypes.c_void_p(d_seg), nRows * nCols, _lib.ptr(rects),
                                                    rects.shape[0], ctypes.c_void_p(_addr(d_table)), nTable, d_packed,
                                                    npacked, bad))
            if bad[0]:
                missing = int(bad[1])
            else:
                packed = numpy.empty((npacked, 4), dtype=numpy.uint8)
                c.check(L.shp_dev_download(c.handle, _lib.ptr(packed), d_packed, packed.nbytes))
    except Exception as e:      # noqa: B902  (raised below, on every rank)
        err = '%s: %s' % (type(e).__name__, e)
    finally:
        if pin is not None:
            tiling._pinnedPut(pin)
        if d_packed is not None:
            tiling._devRelease(c, d_packed, npacked * 4)
    got = comm.allgather_obj((err, missing))
    errs = [(r, g[0]) for (r, g) in enumerate(got) if g[0]]
    if errs:
        raise Err("rendering failed on rank %d: %s" % errs[0])
    labels = [g[1] for g in got if g[1] is not None]
    if labels:
        raise Err("segment id %d is not in the colour table (%d rows)" % (min(labels), nTable))
    if info is not None:
        nBlocks = (nRows + rowsPerBlock - 1) // rowsPerBlock if nCols else 0
        info.update(lookupMs=times[0], downloadMs=times[1], renderMs=times[2], blocks=nBlocks)
    return out, packed


def renderColourTableDistributed(engine, comm, dres, colours=None, outfile=None, overviews=True, blockPixels=None,
                                 info=None):
    """utils.renderColourTable of the label raster that runDistributed(engine, comm, ...) or
    doTiledShepherdSegmentationDistributed(..., keepOutput=True) left sharded over the ranks (``dres`` its
    DistResult), without gathering it: every rank paints the output rows it holds straight from HBM, pixel =
    (Red, Green, Blue, Alpha)[label] (deviceRender; no label leaves the device).

    ``colours``: None -- the table writeColorTableFromRatColumnsDistributed left on the engine --, a
    utils.ColourTableResult, or a mapping with Red, Green, Blue and Alpha (utils._colourColumns; the same on every
    rank, e.g. a seeded utils.writeRandomColourTable(None, dres.maxSegId + 1, seed)).

    ``outfile`` None: returns this rank's (rows (outHi - outLo, nCols, 4) uint8, (outLo, outHi)).  A .npy path
    every rank can write (checkNpyOutfile): rank 0 creates the zero-filled (nRows, nCols, 4) uint8 file, every rank
    pwrites its own pixels -- the pieces of the mosaic it owns, as in writeOutputDistributed, so ranks that share
    output rows (SHEPSEG_SHARD=tiles) work -- and, with ``overviews``, the rectangles its tiles own of
    ``<base>_ov<lvl>.npy`` ((ceil(nRows / lvl), ceil(nCols / lvl), 4), the levels of tiling.overviewLevels): each
    layer is the colour table applied to the label layer writeOutputDistributed writes (rank 0 gives the pixels
    that no tile's block covers the null label's colour: overviewHoles).  Returns None.

    A label without a row in the table raises utils.PyShepSegUtilsError naming the smallest such label of all
    ranks, on every rank; so does a failure while writing.  A rank without output rows joins every collective.
    ``info`` (a dict, optional) receives deviceRender's figures."""
    from . import utils
    Err = utils.PyShepSegUtilsError
    if outfile is not None:
        checkNpyOutfile(outfile)
    err = None
    cols = None
    if not hasattr(engine, 'renderOnDevice'):
        err = "renderColourTableDistributed needs a device engine (HipEngine)"
    elif colours is None:
        if getattr(engine, 'colourTable', None) is None:
            err = "the engine holds no colour table: call writeColorTableFromRatColumnsDistributed first, or pass colours"
    else:
        try:
            cols = utils._colourColumns(colours)
        except Err as e:
            err = str(e)
    distdev.raiseFirst(Err, comm.allgather_obj(err))
    (nRows, nCols) = (dres.nRows, dres.nCols)
    (lo, hi) = dres.outRows
    layers = []
    if outfile is not None and overviews:
        base = outfile[:-4]
        layers = [(int(lvl), base + '_ov%d.npy' % lvl, ((nRows + lvl - 1) // lvl, (nCols + lvl - 1) // lvl))
                  for lvl in tiling.overviewLevels(nCols, nRows)]
    (rects, where, npacked) = (None, [], 0)
    state = {'writer': None}
    sink = None
    if outfile is not None:
        def create():
            if comm.rank == 0:
                for (path, shape) in [(outfile, (nRows, nCols))] + [(p, s) for (_l, p, s) in layers]:
                    tiling._NpyRowWriter(path, shape[0], shape[1], dtype=numpy.uint8, pixelShape=(4,)).close()
        _stepOnAllRanks(comm, outfile, create, Err)
        if layers:
            (rects, where, npacked) = overviewTable(dres, [lvl for (lvl, _p, _s) in layers])
        pieces = _mosaicPieces(dres)

        def sink(y0, y1, rows):             # (rows [y0, y1) of the held block = image rows lo + y0 ...)
            if state['writer'] is None:
                state['writer'] = _NpyRgbaPatchWriter(outfile, nRows, nCols)
            for (a, b, x0, x1) in pieces:
                (ra, rb) = (max(a, lo + y0), min(b, lo + y1))
                if ra < rb:
                    state['writer'].writeRect(ra, x0, rows[ra - lo - y0:rb - lo - y0, x0:x1])
    try:
        (out, packed) = engine.renderOnDevice(comm, cols, rects=rects, npacked=npacked, sink=sink,
                                              blockPixels=blockPixels, info=info)
    finally:
        if state['writer'] is not None:
            state['writer'].close()
    if outfile is None:
        return out, (lo, hi)
    null = numpy.array([col[0] for col in cols], dtype=numpy.uint8) if cols is not None else engine.colourTableRow(0)

    def writeLayers():
        fill = comm.rank == 0 and bool(null.any())
        if not where and not fill:
            return
        files = {lvl: _NpyRgbaPatchWriter(path, *shape) for (lvl, path, shape) in layers}
        try:
            for (q, (lvl, x0, y0, x1, y1)) in zip(rects if where else [], where):
                k = int(q[3] * q[4])
                files[lvl].writeRect(y0, x0, packed[q[5]:q[5] + k].reshape(y1 - y0, x1 - x0, 4))
            # the pixels no block covers hold the null label in the label layer: its colour here (rank 0; no rank
            # owns them, and the file's zeros are that colour already when the table's row 0 is all zero)
            for (lvl, _path, (ovh, ovw)) in (layers if fill else []):
                (holeCols, holeRows) = overviewHoles(dres.tileInfo, dres.overlapSize, lvl)
                for y in holeRows.tolist():
                    files[lvl].writeRect(y, 0, numpy.broadcast_to(null, (1, ovw, 4)))
                for x in holeCols.tolist():
                    files[lvl].writeRect(0, x, numpy.broadcast_to(null, (ovh, 1, 4)))
        finally:
            for f in files.values():
                f.close()
    if layers:
        _stepOnAllRanks(comm, outfile[:-4] + '_ov*.npy', writeLayers, Err)
    return None
