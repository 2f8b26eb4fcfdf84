"""Per-segment spatial statistics on the row-sharded multi-rank output: the built-in user functions as
reductions on the device (deviceSpatialStats, csrc/spatial.h: shp_dspatial_*) and user-defined functions over
point lists built on the device (_userFuncSpatialStats, csrc/dsegpoints.h)."""
import contextlib
import ctypes

import numpy

from . import _lib
from . import distdev
from . import tiling
from .distdev import idRange, spatialHaloPlan, _DTYPE_SIZE


def calcPerSegmentSpatialStatsDistributed(engine, comm, hist, imgbandnum, colTypes, userFunc, userParam,
                                          missingStatsValue=-9999, imgNullVal=None, info=None,
                                          tileSize=tiling.TILESIZE, batchPoints=None):
    """Per-segment spatial statistics (tilingstats.calcPerSegmentSpatialStats) of one image band against the
    label raster that runDistributed left sharded by rows over the ranks.

    A user function (tilingstats.spatialUserFunc, or @jit / @njit) is called once per segment with at least one
    point, with the same ``pts`` as on one GPU: its points in the visit order of ``tileSize`` x ``tileSize``
    tiles of the WHOLE raster.  A segment whose pixels all lie on one rank is called there; a segment with
    pixels on several ranks (a straddler) is called by the rank whose id share (idRange) holds its id, after
    its points have travelled as records.  Each rank makes its calls in ascending id order, in batches of at
    most ``batchPoints`` points (tilingstats.iterSegmentPoints); the ranks call at the same time.  An
    exception of the function on one rank is re-raised there; the other ranks raise PyShepSegStatsError
    naming that rank.  ``info`` receives 'path' = 'points', 'straddlers', 'points_exchanged' (of all ranks)
    and 'calls' (this rank's).

    The built-in user functions run as reductions on the device instead.  As in
    calcPerSegmentStatsDistributed, ``hist`` (DistResult.hist) plays the part of segSize: segments complete on a
    rank are finished there, the straddlers' partial sums travel as packed records and every rank reduces those
    of its id share (idRange).  Edge pixels and the variogram also read rows of the neighbouring ranks (halo
    rows, spatialHaloPlan): they need disjoint output rows (SHEPSEG_SHARD=rows; mean coordinates do not).
    Needs a device engine (HipEngine.spatialOnDevice); a communicator that is not on the device carries the
    device buffers through the host (comm.HostStagedDev).  ``info`` (a dict, optional) receives 'straddlers'
    (segments), 'halo_rows' (of all ranks) and 'path'.  Returns (intcols int64 (nInt, maxSegId+1), floatcols
    float32 (nFloat, maxSegId+1)) on every rank -- bit-identical to calcPerSegmentSpatialStats of the whole
    raster: every accumulator is an integer sum, so the ranks' partial sums add up exactly."""
    from . import tilingstats
    if not hasattr(engine, 'spatialOnDevice'):
        raise tilingstats.PyShepSegStatsError("the distributed spatial statistics need a device engine (HipEngine)")
    dcomm = distdev.deviceComm(comm, engine.c)
    if not isinstance(userFunc, tilingstats._BuiltinSpatialFunc) and tilingstats._isUserFunc(userFunc):
        pinfo = {}
        (ic, fc, nStrad, haloRows) = engine.spatialOnDevice(dcomm, hist, imgbandnum, colTypes, userFunc, userParam,
                                                            missingStatsValue, imgNullVal, tileSize=tileSize,
                                                            batchPoints=batchPoints, info=pinfo)
        if info is not None:
            info.update(pinfo)
        return ic, fc
    (ic, fc, nStrad, haloRows) = engine.spatialOnDevice(dcomm, hist, imgbandnum, colTypes, userFunc, userParam,
                                                        missingStatsValue, imgNullVal, tileSize=tileSize)
    if info is not None:
        info.update(straddlers=nStrad, halo_rows=haloRows, path='device')
    return ic, fc


def deviceSpatialStats(c, comm, d_seg, d_band, dtypeCode, nRows, nCols, rowRange, hist, colTypes, userFunc, userParam,
                       missing=-9999, imgNullVal=None, fetch=True, tileSize=tiling.TILESIZE, batchPoints=None,
                       info=None):
    """The device-resident data path of calcPerSegmentSpatialStatsDistributed for ONE rank: output rows rowRange =
    (outLo, outHi) of an nRows x nCols raster (nRows None: the largest outHi of the ranks), labels d_seg (uint32)
    and band d_band (dtypeCode; -1 on a rank without rows: the other ranks' code) in the HBM of context ``c``;
    comm: allgather_obj, allgather_dev, allreduce_dev_i64.  ``hist``: the global histogram, a numpy array or
    ('dev', address, length).  Halo rows (spatialHaloPlan) travel in one all-gather of labels and one of band
    values; shp_dspatial_local_dev -> all-gather of the straddlers' records -> shp_dspatial_merge_dev by id share
    -> all-reduce of the column block.  Every error that depends on a rank's data is all-gathered first, so all
    ranks raise it.  Returns (ic, fc, straddling segments, halo rows of all ranks); fetch=False: ic = fc = None.
    A user function (tilingstats._isUserFunc) takes the point-list path instead (_userFuncSpatialStats:
    ``tileSize``, ``batchPoints``; ``info`` receives its figures; no halo rows)."""
    from . import tilingstats
    Err = tilingstats.PyShepSegStatsError
    L = c._L
    params = numpy.zeros(6, dtype=numpy.float64)
    pv = numpy.atleast_1d(numpy.asarray(0 if userParam is None else userParam, dtype=numpy.float64))
    params[:min(len(pv), 6)] = pv[:6]
    nInt = sum(1 for t in colTypes if t == tilingstats.GFT_Integer)
    nFloat = sum(1 for t in colTypes if t == tilingstats.GFT_Real)
    func = getattr(userFunc, 'funcId', None) if isinstance(userFunc, tilingstats._BuiltinSpatialFunc) else None
    isUser = func is None and tilingstats._isUserFunc(userFunc)
    err = None
    if func is None and not isUser:
        err = ("userFunc must be one of the built-in user functions (userFuncMeanCoord, userFuncNumEdgePixels, "
               "userFuncVariogram), or a function decorated with tilingstats.spatialUserFunc (or @jit / @njit)")
    elif imgNullVal is None:
        err = "NoData value must be set on imgfile"
    elif nInt + nFloat != len(colTypes) or not colTypes:
        err = "column types must be GFT_Integer or GFT_Real, one or more of them"
    elif func == 2 and not (1.0 <= params[0] <= 255.0):
        err = "variogram maxDist must be 1..255 (got %g)" % params[0]
    elif isUser and int(tileSize) < 1:
        err = "tileSize must be positive"
    ctrl = comm.allgather_obj((int(rowRange[0]), int(rowRange[1]), int(dtypeCode), err, isUser))
    distdev.raiseFirst(Err, [x[3] for x in ctrl])
    if len({x[4] for x in ctrl}) != 1:
        raise Err("the ranks pass different kinds of user function (built-in on some, user-defined on others)")
    ranges = [(x[0], x[1]) for x in ctrl]
    codes = {x[2] for x in ctrl if x[2] >= 0}
    if len(codes) != 1:
        raise Err("the ranks' bands differ in data type (%s)" % sorted(codes))
    dtypeCode = codes.pop()
    isz = _DTYPE_SIZE[dtypeCode]
    nRows = distdev.allRows(ranges, nRows)
    if isUser:
        return _userFuncSpatialStats(c, comm, d_seg, d_band, dtypeCode, nRows, nCols, rowRange, hist, nInt,
                                     nFloat, userFunc, userParam, missing, imgNullVal, fetch, int(tileSize),
                                     batchPoints, info)
    (above, below) = {0: (0, 0), 1: (1, 1), 2: (0, int(params[0]))}[func]
    plan = spatialHaloPlan(ranges, comm.rank, nRows, above, below)     # (raises alike on every rank)
    (lo, hi) = (int(rowRange[0]), int(rowRange[1]))
    h = max(hi - lo, 0)
    (ha, hb) = (plan['above'], plan['below'])
    with distdev.Scratch(c) as s:
        (d_hist, ns, _h32) = distdev.residentHist(s, c, hist)
        S = ns - 1
        colWords = distdev.colWords(nInt, nFloat, ns)
        d_cols = distdev.allocColumns(s, c, colWords)
        # ---- halo rows: every rank's first / last rows in one all-gather of labels and one of band values
        halo = {'segUp': None, 'bandUp': None, 'segDn': None, 'bandDn': None}
        slot = plan['slot']
        if slot and comm.world > 1:
            rowB = (nCols * 4, nCols * isz)
            sends = [s.alloc(max(slot * nCols * b, 1)) for b in rowB]
            alls = [s.alloc(max(comm.world * slot * nCols * b, 1)) for b in rowB]
            for (ownRow, slotRow, n) in plan['send']:
                for (k, src) in enumerate((d_seg, d_band)):
                    c.check(L.shp_dev_copy(c.handle, ctypes.c_void_p(sends[k].value + slotRow * rowB[k]),
                                           ctypes.c_void_p(src + ownRow * rowB[k]), n * rowB[k]))
            for k in range(2):
                comm.allgather_dev(sends[k].value, alls[k].value, slot * rowB[k])
            for (key, rows, recv) in (('Up', ha, plan['recvAbove']), ('Dn', hb, plan['recvBelow'])):
                if not rows:
                    continue
                bufs = [s.alloc(rows * b) for b in rowB]
                halo['seg' + key], halo['band' + key] = bufs
                for (dstRow, src, slotRow, n) in recv:
                    for k in range(2):
                        c.check(L.shp_dev_copy(c.handle, ctypes.c_void_p(bufs[k].value + dstRow * rowB[k]),
                                               ctypes.c_void_p(alls[k].value + (src * slot + slotRow) * rowB[k]),
                                               n * rowB[k]))
        # ---- own rows, the straddlers' records
        (pRec, nRec, W) = (ctypes.c_void_p(), ctypes.c_int64(0), ctypes.c_int64(0))
        checks = numpy.zeros(3, dtype=numpy.int64)
        c.check(L.shp_dspatial_local_dev(
            c.handle, ctypes.c_void_p(d_seg if h else None), ctypes.c_void_p(d_band if h else None), dtypeCode, h,
            nCols, halo['segUp'], halo['bandUp'], ha, halo['segDn'], halo['bandDn'], hb, lo if h else 0, nRows, S,
            int(imgNullVal), func, _lib.ptr(params), int(missing), nInt, nFloat, d_hist, int(comm.rank == 0), d_cols,
            ctypes.byref(pRec), ctypes.byref(nRec), ctypes.byref(W), _lib.ptr(checks)))
        flagged = [_varioPairs(c)] if func == 2 else []
        got = comm.allgather_obj((int(nRec.value), [int(x) for x in checks]))
        distdev.raiseFirst(Err, [distdev.histogramMismatch(sum(g[1][0] for g in got), sum(g[1][1] for g in got),
                                                           got[0][1][2])])
        counts = [g[0] for g in got]
        nIds = ctypes.c_int64(0)
        (d_all, recSlot) = distdev.gatherRecords(s, c, comm, pRec, nRec.value, counts, int(W.value) * 8)
        if recSlot > 0:
            (idLo, idHi) = idRange(comm.rank, comm.world, S)
            cnts = numpy.array(counts, dtype=numpy.uint32)
            c.check(L.shp_dspatial_merge_dev(c.handle, d_all, recSlot, comm.world, _lib.ptr(cnts), S, func,
                                             _lib.ptr(params), int(missing), nInt, nFloat, idLo, idHi, d_cols,
                                             ctypes.byref(nIds)))
            if func == 2:
                flagged.append(_varioPairs(c))
        if func == 2:
            nRedo = _varioRedo(c, comm, ranges, flagged, d_seg if h else None, d_band if h else None, dtypeCode, h, nCols,
                               halo['segDn'], halo['bandDn'], hb, S, imgNullVal, int(params[0]), nInt, nFloat,
                               d_cols)
            if info is not None:
                info['varioRecomputed'] = nRedo
        if comm.world > 1:
            comm.allreduce_dev_i64(d_cols.value, colWords)
        (ic, fc) = distdev.fetchColumns(c, d_cols, nInt, nFloat, ns, fetch)
    tot = comm.allgather_obj((int(nIds.value), ha + hb))
    return ic, fc, int(sum(t[0] for t in tot)), int(sum(t[1] for t in tot))


def _varioPairs(c):
    """The flagged variogram pairs (s * maxDist + bin) of the context's last local or merge step (uint64)."""
    n = ctypes.c_int64(0)
    c.check(c._L.shp_dspatial_vario_pairs(c.handle, None, 0, ctypes.byref(n)))
    out = numpy.zeros(n.value, dtype=numpy.uint64)
    if n.value:
        c.check(c._L.shp_dspatial_vario_pairs(c.handle, _lib.ptr(out), n.value, ctypes.byref(n)))
    return out


def _varioRedo(c, comm, ranges, flagged, d_seg, d_band, dtypeCode, h, nCols, segDn, bandDn, hb, S, imgNullVal, maxDist,
               nInt, nFloat, d_cols):
    """The variogram pairs flagged on any rank (the union of ``flagged``, every rank's local and merge flags),
    recomputed in the reference's order: rank after rank from the top of the image (``ranges``: every rank's
    output rows), each continuing the sums and counts over its own rows; rank 0 stores the pairs' entries into d_cols and the others zero them, so that the
    sum of the column blocks holds them.  Returns the number of pairs."""
    mine = numpy.concatenate(flagged) if flagged else numpy.zeros(0, dtype=numpy.uint64)
    pairs = numpy.unique(numpy.concatenate(comm.allgather_obj(mine)).astype(numpy.uint64))
    n = len(pairs)
    if n == 0:
        return 0
    (sums, cnts) = (numpy.zeros(n, dtype=numpy.float64), numpy.zeros(n, dtype=numpy.uint32))
    for r in sorted(range(comm.world), key=lambda k: (ranges[k][0], k)):
        if r == comm.rank and h:
            c.check(c._L.shp_dspatial_vario_redo_dev(
                c.handle, ctypes.c_void_p(d_seg), ctypes.c_void_p(d_band), dtypeCode, h, nCols, segDn, bandDn, hb,
                S, int(imgNullVal), maxDist, _lib.ptr(pairs), n, _lib.ptr(sums), _lib.ptr(cnts)))
        if comm.world > 1:
            (sums, cnts) = comm.allgather_obj((sums, cnts) if r == comm.rank else None)[r]
            (sums, cnts) = (numpy.ascontiguousarray(sums), numpy.ascontiguousarray(cnts))
    c.check(c._L.shp_dspatial_vario_store_dev(c.handle, _lib.ptr(pairs), n, _lib.ptr(sums), _lib.ptr(cnts),
                                              maxDist, S, nInt, nFloat, d_cols, int(comm.rank == 0)))
    return n


SEGPOINT_RECORD_BYTES = 24         # a straddler's point as it travels: visit index, id, x, y, value bits


def userFuncRowPlan(hist, localLabels, localPoints, share, merged, pointless):
    """Which rows of the columns one rank answers for in the user-function path of deviceSpatialStats (host only).
    hist: the global histogram (S + 1); localLabels / localPoints: labelled pixels / points (non-nodata pixels)
    of every id on this rank; share = (idLo, idHi), this rank's id share (idRange); merged: points of every id
    of the share that reached this rank as records (idHi - idLo); pointless: ids that straddle ranks and have no
    point on some rank that reported them (every rank's list together).
    A row belongs to the rank that holds all of the id's pixels (complete: local count == hist) or, for ids that
    no rank holds completely -- straddlers, and ids without pixels -- to the owner of the id's share.  So every
    row has exactly one owner, which the column all-reduce needs.  Returns (emit, owned, straddlers): emit
    (int64, S + 1) = the points this rank hands the function for every id (an id with emit > 0 is called here,
    once), owned (bool, S + 1) = the rows it writes, straddlers = the straddling ids of its share."""
    hist = numpy.asarray(hist, dtype=numpy.int64)
    lh = numpy.asarray(localLabels, dtype=numpy.int64)
    lp = numpy.asarray(localPoints, dtype=numpy.int64)
    merged = numpy.asarray(merged, dtype=numpy.int64)
    (lo, hi) = (int(share[0]), int(share[1]))
    complete = (lh == hist) & (hist > 0)
    complete[:1] = False
    emit = numpy.where(complete, lp, 0)
    owned = complete.copy()
    nStrad = 0
    if hi > lo:
        strad = (merged > 0) | numpy.isin(numpy.arange(lo, hi), numpy.asarray(pointless, dtype=numpy.int64))
        owned[lo:hi] |= (hist[lo:hi] == 0) | strad
        emit[lo:hi] += merged
        nStrad = int(numpy.count_nonzero(strad))
    emit[:1] = 0
    return emit, owned, nStrad


def clearUnownedRows(intcols, floatcols, owned):
    """The missing-value fill of the user-function path: runUserFunc left missingStatsValue in every row it did
    not call for (row 0 zero); the rows this rank does not own become zero, so that the ranks' column blocks
    add up to the one-GPU columns (each row written by one rank, every 32-bit half with one non-zero
    contributor)."""
    intcols[:, ~owned] = 0
    floatcols[:, ~owned] = 0
    return intcols, floatcols


def userFuncErrorOf(gathered):
    """The error every rank raises after the user-function calls: gathered = every rank's None or (exception
    type name, message).  Returns None or the message for the ranks whose own calls did not fail."""
    for (r, g) in enumerate(gathered):
        if g is not None:
            return "the spatial user function raised %s on rank %d: %s" % (g[0], r, g[1])
    return None


def _userFuncSpatialStats(c, comm, d_seg, d_band, dtypeCode, nRows, nCols, rowRange, hist, nInt, nFloat,
                          userFunc, userParam, missing, imgNullVal, fetch, tileSize, batchPoints, info):
    """The user-function path of deviceSpatialStats (after its control exchange): shp_dsegpoints_build_dev over
    the own rows -> all-gather of the straddlers' point records -> shp_dsegpoints_merge_dev of this rank's id
    share -> tilingstats.runUserFunc over this rank's batches (ids complete here and straddlers of the share, in
    ascending id order) -> all-reduce of the column block.  The point lists live in a context of their own
    (each of its calls needs the previous one's workspace); copies, collectives and pinned buffers use ``c``."""
    from . import tilingstats
    Err = tilingstats.PyShepSegStatsError
    L = c._L
    (lo, hi) = (int(rowRange[0]), int(rowRange[1]))
    h = max(hi - lo, 0)
    # (the scratch goes back before the second context closes)
    with contextlib.closing(_lib.Context(device=c.device)) as pc, distdev.Scratch(c) as s:
        (d_hist, ns, h32) = distdev.residentHist(s, c, hist, host=True)
        S = ns - 1
        PL = pc._L
        (lh, lp) = (numpy.zeros(ns, dtype=numpy.uint32), numpy.zeros(ns, dtype=numpy.uint32))
        (pRec, nRec) = (ctypes.c_void_p(), ctypes.c_int64(0))
        pc.check(PL.shp_dsegpoints_build_dev(
            pc.handle, ctypes.c_void_p(d_seg if h else None), ctypes.c_void_p(d_band if h else None), dtypeCode, h,
            nCols, lo if h else 0, nRows, S, int(imgNullVal), tileSize, d_hist, _lib.ptr(lh), _lib.ptr(lp),
            ctypes.byref(pRec), ctypes.byref(nRec)))
        # ---- the histogram's checks and the straddlers without points, of every rank
        hist64 = h32.astype(numpy.int64)
        strad = (lh > 0) & (lh.astype(numpy.int64) < hist64)
        over = int(numpy.count_nonzero(lh.astype(numpy.int64) > hist64))
        pointless = numpy.flatnonzero(strad & (lp == 0)).astype(numpy.uint32)
        got = comm.allgather_obj((int(nRec.value), over, int(lh.sum(dtype=numpy.int64)), pointless))
        distdev.raiseFirst(Err, [distdev.histogramMismatch(sum(g[1] for g in got), sum(g[2] for g in got),
                                                           int(hist64[1:].sum()))])
        counts = [g[0] for g in got]
        (idLo, idHi) = idRange(comm.rank, comm.world, S)
        (d_all, slot) = distdev.gatherRecords(s, c, comm, pRec, nRec.value, counts, SEGPOINT_RECORD_BYTES)
        merged = numpy.zeros(max(idHi - idLo, 1), dtype=numpy.uint32)
        nMerged = ctypes.c_int64(0)
        cnts = numpy.array(counts, dtype=numpy.uint32)
        pc.check(PL.shp_dsegpoints_merge_dev(pc.handle, d_all, slot, comm.world, _lib.ptr(cnts), idLo, idHi,
                                             _lib.ptr(merged), ctypes.byref(nMerged)))
        merged = merged[:idHi - idLo]
        allPointless = numpy.concatenate([numpy.asarray(g[3], dtype=numpy.int64) for g in got])
        (ecnt, owned, nStradMine) = userFuncRowPlan(hist64, lh, lp, (idLo, idHi), merged, allPointless)
        # ---- this rank's calls, batch by batch (the ids complete here, the straddlers of the share)
        batches = tilingstats.planPointBatches(ecnt, tilingstats.POINTS_BATCH if batchPoints is None else batchPoints)
        cum = numpy.concatenate([[0], numpy.cumsum(ecnt, dtype=numpy.int64)])
        cap = max([int(cum[b] - cum[a]) for (a, b) in batches] + [1])
        hostBufs = [tilingstats._PinnedBuffer(c, cap * tilingstats.SEGPOINT_DTYPE.itemsize)
                    for _k in range(min(2, len(batches)))]

        def emit(a, b, offs, buf, n):
            pc.check(PL.shp_dsegpoints_emit(pc.handle, a, b, _lib.ptr(offs), buf, cap, ctypes.byref(n)))
            if n.value != int(cum[b] - cum[a]):
                raise Err("internal: ids %d..%d emitted %d points, %d planned" % (a, b, n.value, int(cum[b] - cum[a])))
        failed = None
        try:
            with contextlib.closing(tilingstats.emitPointBatches(batches, hostBufs, emit)) as it:
                (ic, fc) = tilingstats.runUserFunc(it, ns, userFunc, userParam, imgNullVal, nInt, nFloat, missing)
        except Exception as e:      # (every rank learns of it before anyone leaves the collectives)
            failed = e
        errs = comm.allgather_obj(None if failed is None else (type(failed).__name__, str(failed)))
        if failed is not None:
            raise failed
        distdev.raiseFirst(Err, [userFuncErrorOf(errs)])
        clearUnownedRows(ic, fc, owned)
        # ---- the column block: the ranks' rows add up
        if comm.world > 1:
            colWords = distdev.colWords(nInt, nFloat, ns)
            block = numpy.zeros(colWords * 8, dtype=numpy.uint8)
            block[:ic.nbytes] = ic.reshape(-1).view(numpy.uint8)
            block[ic.nbytes:ic.nbytes + fc.nbytes] = fc.reshape(-1).view(numpy.uint8)
            d_cols = s.alloc(colWords * 8)
            c.check(L.shp_dev_upload(c.handle, d_cols, _lib.ptr(block), block.nbytes))
            comm.allreduce_dev_i64(d_cols.value, colWords)
            c.check(L.shp_dev_download(c.handle, _lib.ptr(block), d_cols, block.nbytes))
            ic = block[:ic.nbytes].view(numpy.int64).reshape(nInt, ns).copy()
            fc = block[ic.nbytes:ic.nbytes + fc.nbytes].view(numpy.float32).reshape(nFloat, ns).copy()
    # the job's figures: the ranks' id shares partition the straddlers
    tot = comm.allgather_obj((nStradMine, int(nRec.value)))
    nStrad = int(sum(t[0] for t in tot))
    if info is not None:
        info.update(path='points', straddlers=nStrad, points_exchanged=int(sum(t[1] for t in tot)),
                    calls=int(numpy.count_nonzero(ecnt)))
    if not fetch:
        (ic, fc) = (None, None)
    return ic, fc, nStrad, 0
