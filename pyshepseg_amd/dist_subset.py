"""subset.subsetImage of the row-sharded multi-rank output (deviceSubset, csrc/dsubset.h: shp_dsubset_*)."""
import ctypes

import numpy

from . import _lib
from . import distdev
from . import tiling
from .distdev import disjointRowsError, _writeRows


def subsetHeldRows(rowRange, tly, ys):
    """The window rows [a, b) that output rows rowRange = (outLo, outHi) hold of a window of ys rows from image
    row tly: [max(0, outLo - tly), min(ys, outHi - tly)), as (a, a) when they hold none (host only)."""
    (lo, hi, tly, ys) = (int(rowRange[0]), int(rowRange[1]), int(tly), int(ys))
    a = min(max(0, lo - tly), ys)
    return a, max(a, min(ys, hi - tly))


def deviceSubset(c, comm, d_seg, nRows, nCols, rowRange, maxSegId, tlx, tly, xs, ys, mask=None, tileSize=None,
                 info=None):
    """The device-resident data path of subsetImageDistributed for ONE rank: output rows rowRange = (outLo, outHi)
    of an nRows x nCols label raster (nRows None: the largest outHi of the ranks) at d_seg (uint32) in the HBM of
    context ``c``; comm: allgather_obj, allgather_dev, allreduce_dev_i64.  The window (tlx, tly, xs, ys), ``mask``
    (None, an array or a .npy path of shape (ys, xs)) and ``tileSize`` mean what they mean in subset.subsetImage;
    maxSegId bounds the labels (DistResult.maxSegId).
    shp_dsubset_local_dev finds the first-seen key of every id in the window rows this rank holds
    (subsetHeldRows) -> one all-gather of the (key, id) pairs, padded to the largest count -> every rank runs the
    same shp_dsubset_merge_dev (the same numbering everywhere) and recodes its rows -> one all-reduce of the
    histogram.  Every error that depends on a rank's data is all-gathered first, so all ranks raise it.
    Returns (rows (b - a, xs) uint32 on the host, (a, b), origSegIds, hist); the last two are the same on every
    rank and equal subset.subsetImage's.  ``info`` (a dict, optional) receives 'pairs' (of all ranks)."""
    from . import subset
    Err = subset.PyShepSegSubsetError
    (tlx, tly, xs, ys) = (int(tlx), int(tly), int(xs), int(ys))
    tileSize = tiling.TILESIZE if tileSize is None else int(tileSize)
    ranges = [(int(a), int(b)) for (a, b) in comm.allgather_obj((int(rowRange[0]), int(rowRange[1])))]
    nRows = distdev.allRows(ranges, nRows)
    err = disjointRowsError(ranges, 'subsetImageDistributed')
    maskArr = None
    try:
        if err is None:
            subset.checkWindow(nRows, int(nCols), tlx, tly, xs, ys)
            maskArr = subset.loadMask(mask, xs, ys)
            if tileSize < 1:
                err = "tileSize must be positive"
    except Err as e:
        err = str(e)
    distdev.raiseFirst(Err, comm.allgather_obj(err))
    L = c._L
    (lo, hi) = ranges[comm.rank]
    (a, b) = subsetHeldRows((lo, hi), tly, ys)
    h = max(hi - lo, 0)
    with distdev.Scratch(c) as s:
        d_mask = None
        if maskArr is not None and b > a:
            part = numpy.ascontiguousarray(maskArr[a:b])
            d_mask = s.alloc(part.nbytes)
            c.check(L.shp_dev_upload(c.handle, d_mask, _lib.ptr(part), part.nbytes))
        geom = (ctypes.c_void_p(d_seg if h else None), h, int(nCols), lo if h else 0, int(maxSegId), tlx, tly, xs, ys,
                tileSize, d_mask)
        (pPairs, nPairs, bad) = (ctypes.c_void_p(), ctypes.c_int64(0), ctypes.c_int(0))
        c.check(L.shp_dsubset_local_dev(c.handle, *geom, ctypes.byref(pPairs), ctypes.byref(nPairs),
                                        ctypes.byref(bad)))
        got = comm.allgather_obj((int(nPairs.value), int(bad.value)))
        badRanks = [r for (r, g) in enumerate(got) if g[1]]
        if badRanks:
            raise Err("segment id above maxSegId (%d) in the subset (rank %s)" % (int(maxSegId),
                                                                                  ', '.join(map(str, badRanks))))
        counts = [g[0] for g in got]
        if sum(counts) == 0:
            raise Err('No valid data found in subset')
        (d_all, slot) = distdev.gatherRecords(s, c, comm, pPairs, nPairs.value, counts, 8)
        # hist as uint32 lanes of int64 words: no id has 2^32 pixels in the window, so no carry crosses a lane
        cap = sum(counts) + 1
        cap += cap % 2
        d_hist = s.alloc(cap * 4)
        d_rows = s.alloc((b - a) * xs * 4)
        orig = numpy.zeros(cap, dtype=numpy.uint32)
        nNew = ctypes.c_uint32(0)
        cnts = numpy.array(counts, dtype=numpy.uint32)
        c.check(L.shp_dsubset_merge_dev(c.handle, d_all, slot, comm.world, _lib.ptr(cnts), *geom, d_rows, d_hist,
                                        _lib.ptr(orig), cap, ctypes.byref(nNew)))
        m = int(nNew.value)
        words = (m + 2) // 2
        if comm.world > 1:
            comm.allreduce_dev_i64(d_hist.value, words)
        hist = numpy.zeros(2 * words, dtype=numpy.uint32)
        c.check(L.shp_dev_download(c.handle, _lib.ptr(hist), d_hist, hist.nbytes))
        rows = numpy.empty((b - a, xs), dtype=numpy.uint32)
        if rows.size:
            c.check(L.shp_dev_download(c.handle, _lib.ptr(rows), d_rows, rows.nbytes))
    if info is not None:
        info['pairs'] = int(sum(counts))
    return rows, (a, b), orig[:m + 1].copy(), hist[:m + 1].copy()


def subsetImageDistributed(engine, comm, result, tlx, tly, newXsize, newYsize, outname=None, origSegIdColName=None,
                           maskImage=None, ratColumns=None, tileSize=None):
    """subset.subsetImage of the label raster that runDistributed(engine, comm, ...) left sharded by rows over the
    ranks (a HipEngine(keepOutput=True); ``result`` its DistResult), without gathering it: every rank recodes
    the window rows it holds (deviceSubset).  Arguments as subset.subsetImage; ``outname`` None or a .npy path
    every rank can write: rank 0 creates it, every rank writes its rows.  Returns a subset.SubsetResult: segimg =
    this rank's rows of the recoded window, rows = (a, b) the window rows they are; origSegIds, hist and columns
    are the same on every rank and equal subset.subsetImage's of the whole raster.  Errors are raised on every
    rank.  Output rows shared by several ranks (SHEPSEG_SHARD=tiles) are refused."""
    from . import subset
    Err = subset.PyShepSegSubsetError
    err = None
    if not hasattr(engine, 'subsetOnDevice'):
        err = "subsetImageDistributed needs a device engine (HipEngine)"
    elif outname is not None:
        try:
            subset.checkOutname(outname)
        except Err as e:
            err = str(e)
    distdev.raiseFirst(Err, comm.allgather_obj(err))
    dcomm = distdev.deviceComm(comm, engine.c)
    (rows, (a, b), orig, hist) = engine.subsetOnDevice(dcomm, result.maxSegId, tlx, tly, newXsize, newYsize,
                                                       mask=maskImage, tileSize=tileSize)
    res = subset.SubsetResult()
    (res.segimg, res.rows, res.origSegIds, res.hist) = (rows, (a, b), orig, hist)
    res.columns = subset.recodeColumns(orig, hist, ratColumns, origSegIdColName)
    if outname is not None:
        _writeRows(comm, outname, rows, a, (int(newYsize), int(newXsize)))
    return res
