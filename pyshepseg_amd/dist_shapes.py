"""Per-segment shape attributes of the row-sharded multi-rank output (calcSegmentShapesDistributed) and their device
path for ONE rank (deviceShapes, csrc/dsegshape.h): shapes.calcSegmentShapes of the whole mosaic, bit for bit, without
gathering the labels."""
import ctypes
import time

import numpy

from . import _lib
from . import distdev
from .distdev import idRange, spatialHaloPlan, disjointRowsError, _rowsCoverError

# bytes of a straddler's record: the id and the eleven words of its row (csrc/dsegshape.h)
SHAPE_RECORD_BYTES = 96


def deviceShapes(c, comm, d_seg, nRows, nCols, rowRange, maxSegId, hist, missingStatsValue=-9999, info=None):
    """The device-resident data path of calcSegmentShapesDistributed for ONE rank, the counterpart of
    dist_neighbours.deviceNeighbours with its arguments: output rows rowRange = (outLo, outHi) of an nRows x nCols label
    raster (nRows None: the largest outHi of the ranks) at d_seg (uint32) in the HBM of context ``c``; comm:
    allgather_obj, allgather_dev, allreduce_dev_i64.  maxSegId bounds the labels and is the table's last row.  ``hist``:
    the whole raster's pixel count per id (maxSegId + 1 values; row 0 is not compared), a numpy array or ('dev', address,
    length) when it is in device memory already (distdev.residentHist).

    Every rank all-gathers its first and its last row (spatialHaloPlan: thin and empty shards, the raster's rim) and
    accumulates its rows with the row above and below them where they lie in the gathered buffer
    (shp_shape_accumulate_halo_dev), coordinates counted from the whole raster's origin.  An id whose area here is
    hist[id] is whole on this rank; the rows of the others -- the segments that straddle a cut -- leave the table as
    96-byte records (shp_dshape_local_dev) and travel in one all-gather, slot = the largest count of the ranks.  Every
    rank folds the records of the ids of its share (idRange) into its table (shp_dshape_merge_dev: sums and counts add,
    extents combine by min / max), after which an id's row is non-zero on at most one rank, and one integer all-reduce
    of the (maxSegId + 1) x 11 words completes the table everywhere.  The float columns come from
    shapes.shapeColumnsFromSums on the host, as on one GPU.

    Control data travels first, so every error that depends on a rank's data is raised on every rank
    (shapes.PyShepSegShapesError): a label above maxSegId (the one-GPU message, with the largest label over all ranks),
    output rows shared by several ranks (SHEPSEG_SHARD=tiles), a histogram that is not these labels' (an id with more
    pixels on a rank than it gives the id, or with another area after the exchange).

    Returns a shapes.SegmentShapes, complete and the same on every rank.  ``info`` (a dict, optional) receives
    'halo_rows' (of all ranks), 'records_sent' (this rank's straddlers), 'records_picked' (folded here, this rank's own
    among them), 'straddlers' (distinct straddling ids over all ranks) and 'exchange_bytes' (96 x the records of all
    ranks + 8 nCols x the ranks that hold rows: what every rank receives; 0 at world 1)."""
    from . import shapes
    Err = shapes.PyShepSegShapesError
    t0 = time.perf_counter()
    err = None
    try:
        if int(maxSegId) != maxSegId or maxSegId < 0 or maxSegId >= 0xFFFFFFFE:
            err = "maxSegId must be an integer in 0..2^32 - 3 (got {})".format(maxSegId)
    except (TypeError, ValueError):
        err = "maxSegId must be an integer (got {!r})".format(maxSegId)
    nHist = int(hist[2]) if isinstance(hist, tuple) else len(hist)
    if err is None and nHist != int(maxSegId) + 1:
        err = "the histogram has {} rows, maxSegId + 1 = {}".format(nHist, int(maxSegId) + 1)
    ctrl = comm.allgather_obj((int(rowRange[0]), int(rowRange[1]), err, None if err else int(maxSegId),
                               int(nCols)))                                                   # control data
    distdev.raiseFirst(Err, [x[2] for x in ctrl])
    if len({x[3:] for x in ctrl}) != 1:
        raise Err("the ranks pass different maxSegId or columns: %s" % sorted({x[3:] for x in ctrl}))
    (S, nCols, d_seg) = (int(maxSegId), int(nCols), distdev._addr(d_seg))
    ranges = [(x[0], x[1]) for x in ctrl]
    nRows = distdev.allRows(ranges, nRows)
    distdev.raiseFirst(Err, [disjointRowsError(ranges, 'calcSegmentShapesDistributed') or _rowsCoverError(ranges, nRows)])
    plan = spatialHaloPlan(ranges, comm.rank, nRows, 1, 1)
    (lo, hi) = ranges[comm.rank]
    h = max(hi - lo, 0)
    (idLo, idHi) = idRange(comm.rank, comm.world, S)
    L = c._L
    timings = {}
    ms = ctypes.c_double(0)
    with distdev.Scratch(c) as s:
        (d_hist, ns, _h32) = distdev.residentHist(s, c, hist)
        # ---- the halo rows: every rank's first and last row in one all-gather
        (d_above, d_below) = (None, None)
        rowB = nCols * 4
        holders = 0
        if comm.world > 1 and nCols > 0:
            d_send = s.alloc(2 * rowB)
            d_rows = s.alloc(comm.world * 2 * rowB)
            for (ownRow, slotRow, _n) in plan['send']:
                c.check(L.shp_dev_copy(c.handle, ctypes.c_void_p(d_send.value + slotRow * rowB),
                                       ctypes.c_void_p(d_seg + ownRow * rowB), rowB))
            comm.allgather_dev(d_send.value, d_rows.value, 2 * rowB)
            holders = sum(1 for (a, b) in ranges if b > a)
            if plan['recvAbove']:
                (_row, src, slotRow, _n) = plan['recvAbove'][0]
                d_above = ctypes.c_void_p(d_rows.value + (2 * src + slotRow) * rowB)
            if plan['recvBelow']:
                (_row, src, slotRow, _n) = plan['recvBelow'][0]
                d_below = ctypes.c_void_p(d_rows.value + (2 * src + slotRow) * rowB)
        timings['halo'] = time.perf_counter() - t0
        # ---- own rows into a table of all ids, coordinates from the raster's origin
        t1 = time.perf_counter()
        c.check(L.shp_shape_begin(c.handle, S, lo if h else 0, 0))
        if h and nCols:
            c.check(L.shp_shape_accumulate_halo_dev(c.handle, ctypes.c_void_p(d_seg), h, nCols, d_above, d_below))
        timings['accumulate'] = time.perf_counter() - t1
        # ---- whole here, or a straddler's record
        t1 = time.perf_counter()
        (maxLabel, pRec) = (ctypes.c_uint32(0), ctypes.c_void_p())
        cnt = numpy.zeros(2, dtype=numpy.int64)
        c.check(L.shp_dshape_local_dev(c.handle, d_hist, ns, ctypes.byref(maxLabel), _lib.ptr(cnt), ctypes.byref(pRec),
                                       ctypes.byref(ms)))
        got = comm.allgather_obj((int(maxLabel.value), int(cnt[0]), int(cnt[1]), plan['above'] + plan['below']))
        worst = max(g[0] for g in got)
        if worst > S:
            raise Err("segment id {} is above maxSegId {}".format(worst, S))
        over = sum(g[2] for g in got)
        if over:
            raise Err(_histogramError(over, 0))
        timings['local'] = time.perf_counter() - t1
        # ---- the straddlers' records of all ranks
        t1 = time.perf_counter()
        counts = [g[1] for g in got]
        (d_all, slot) = distdev.gatherRecords(s, c, comm, pRec, int(cnt[0]), counts, SHAPE_RECORD_BYTES)
        timings['exchange'] = time.perf_counter() - t1
        # ---- the records of this rank's id share, folded; the table completed
        t1 = time.perf_counter()
        (cnt3, pTab) = (numpy.zeros(3, dtype=numpy.int64), ctypes.c_void_p())
        cnts = numpy.array(counts, dtype=numpy.uint32)
        c.check(L.shp_dshape_merge_dev(c.handle, d_all, slot, comm.world, _lib.ptr(cnts), d_hist, ns, idLo, idHi,
                                       _lib.ptr(cnt3), ctypes.byref(pTab), ctypes.byref(ms)))
        got2 = comm.allgather_obj((int(cnt3[1]), int(cnt3[2])))
        wrong = sum(g[1] for g in got2)
        if wrong:
            raise Err(_histogramError(0, wrong))
        if comm.world > 1:
            comm.allreduce_dev_i64(pTab.value, ns * shapes._TABLE_WORDS)
        timings['merge'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        table = numpy.empty((ns, shapes._TABLE_WORDS), dtype=numpy.uint64)
        c.check(L.shp_shape_download(c.handle, _lib.ptr(table)))
        timings['download'] = time.perf_counter() - t1
    t1 = time.perf_counter()
    (columns, sums) = shapes.columnsFromTable(table, missingStatsValue)
    timings['derive'] = time.perf_counter() - t1
    timings['total'] = time.perf_counter() - t0
    figures = dict(halo_rows=int(sum(g[3] for g in got)), records_sent=int(cnt[0]), records_picked=int(cnt3[0]),
                   straddlers=int(sum(g[0] for g in got2)),
                   exchange_bytes=SHAPE_RECORD_BYTES * int(sum(counts)) + 2 * rowB * holders)
    if info is not None:
        info.update(figures)
    return shapes.SegmentShapes(S, columns, sums, (0, 0), timings=timings, deviceMs=ms.value)


def _histogramError(over, wrong):
    return ("the segment histogram does not match the label raster (%d ids with more pixels on one rank than the "
            "histogram gives them, %d ids whose area over all ranks is not the histogram's)" % (over, wrong))


def calcSegmentShapesDistributed(engine, comm, dres, hist=None, missingStatsValue=-9999, info=None):
    """shapes.calcSegmentShapes of the label raster that lies sharded by rows over the ranks, without gathering it: a
    shapes.SegmentShapes, complete and identical on every rank, whose ``columns`` and ``sums`` equal those of
    calcSegmentShapes(mosaic, origin=(0, 0)) bit for bit (``cols.update(s.columns)``, as with the statistics and the
    neighbour columns).

    ``dres``: the DistResult of runDistributed / doTiledShepherdSegmentationDistributed(keepOutput=True) -- the rows
    are the engine's kept output, ``maxSegId`` and the histogram the result's -- or the neighbours.MergedSegmentsShare
    of mergeSegmentsDistributed / mergeSimilarSegmentsDistributed(..., dres=...): its recoded rows ``outDev`` /
    ``rowRange`` (a rank without rows has outDev None and still takes part), its ``maxSegId`` and ``hist``.  ``hist``
    overrides the object's histogram.  ``engine``: a HipEngine; there is no CPU fallback.  A communicator that is not
    on the device carries the device buffers through the host (comm.HostStagedDev).  ``info`` and the errors raised
    on every rank: see deviceShapes."""
    from . import neighbours, shapes
    Err = shapes.PyShepSegShapesError
    if not hasattr(engine, 'shapesOnDevice'):
        raise Err("the distributed shape attributes need a device engine (HipEngine)")
    if hist is None:
        hist = getattr(dres, 'hist', None)
    if hist is None:
        raise Err("no histogram: %s carries none (a merge without segSize and without dres), and hist is not given"
                  % type(dres).__name__)
    try:
        missing = neighbours._number(missingStatsValue, 'missingStatsValue')
    except neighbours.PyShepSegNeighboursError as e:
        raise Err(str(e))
    dcomm = distdev.deviceComm(comm, engine.c)
    if isinstance(dres, neighbours.MergedSegmentsShare):
        if dres.rowRange is None:
            raise Err("the MergedSegmentsShare holds no recoded rows: run the merge with dres")
        d_seg = int(dres.outDev[0]) if dres.outDev else 0
        return deviceShapes(engine.c, dcomm, d_seg, None, engine.nCols, dres.rowRange, dres.maxSegId, hist, missing, info=info)
    return engine.shapesOnDevice(dcomm, dres.maxSegId, hist, missingStatsValue=missing, info=info)
