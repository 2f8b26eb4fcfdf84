"""Per-segment statistics of image bands on the row-sharded multi-rank output: the split over entries
(_distributedStats: the protocol an engine provides) and its device path for ONE rank (deviceStatsBands,
csrc/segstats.h: shp_dstats_*)."""
import ctypes

import numpy

from . import _lib
from . import distdev
from .distdev import idRange, _raiseOnAllRanks, _raiseFirstError


def calcPerSegmentStatsDistributed(engine, comm, hist, imgbandnum, statsSelection,
                                   missingStatsValue=-9999, imgNullVal=None, info=None):
    """Per-segment statistics of one image band against the stitched label raster that
    runDistributed left sharded by rows over the ranks (reference tilingstats.py:85-216; SURVEY
    8e).  ``hist`` is the global histogram of the labels (DistResult.hist), which plays the part
    of the reference's segSize: a segment whose local pixel count equals hist[id] is complete on
    this rank and its statistics are final (checkSegComplete, tilingstats.py:518-553).  The
    pixels of the segments that straddle a rank boundary are packed, id and value, and
    all-gathered; every rank then reduces the straddlers whose id lies in ITS share of the id space
    (idRange) with the same kernel.  Finished rows are disjoint between ranks, so one integer
    all-reduce assembles the columns.
      This is calcPerSegmentStatsDistributedBands with the one entry (imgbandnum, statsSelection): the same
    driver (_distributedStats), the same transports, the same ``info`` keys; the band number is not checked
    against the image here.  A ``hist`` that gives an id FEWER pixels than a rank holds of it raises on every
    rank: _lib.ShepsegHipError on the device path, tilingstats.PyShepSegStatsError on the host path.
    Returns (intcols int64 (nInt, maxSegId+1), floatcols float32 (nFloat, maxSegId+1),
    statsSelection_fast) on every rank -- bit-identical to the single-GPU result."""
    from . import tilingstats
    statsSelection = list(statsSelection)
    (fast, nInt, nFloat) = tilingstats.makeFastStatsSelection(list(range(len(statsSelection))), statsSelection)
    return _distributedStats(engine, comm, hist, [(int(imgbandnum), statsSelection)], fast,
                             numpy.zeros(len(statsSelection), dtype=numpy.intp), nInt, nFloat, [imgNullVal],
                             missingStatsValue, info)


def deviceStats(c, comm, d_seg, d_band, dtypeCode, nRows, nCols, hist, fast, nInt, nFloat, missing, imgNullVal,
                fetch=True):
    """deviceStatsBands for ONE entry: band rows d_band, selection ``fast``, null value imgNullVal (None: none).  A
    rank without rows (nRows 0) passes any non-zero d_band, which is not read, and may pass dtypeCode None.
    Returns (ic, fc, straddling segments, their pixels)."""
    return deviceStatsBands(c, comm, d_seg, [d_band], dtypeCode, nRows, nCols, hist, fast, [len(fast)],
                            [int(imgNullVal is not None)], [0 if imgNullVal is None else int(imgNullVal)], nInt, nFloat,
                            missing, fetch=fetch)[:4]


def _engineBandCount(engine):
    """How many image bands the engine holds (``numBands``, or the whole image ``img`` of a host engine); None when
    this rank cannot tell (a device engine without rows)."""
    nb = getattr(engine, 'numBands', None)
    if nb is None and getattr(engine, 'img', None) is not None:
        nb = engine.img.shape[0]
    return nb


def _placeEntryColumns(ic, fc, bic, bfc, bfast, combined):
    """The columns of ONE entry, numbered from 0 by its own fast selection ``bfast``, into the rows of the combined
    selection's columns (``combined``: the entry's rows of it)."""
    from . import tilingstats
    for (own, comb) in zip(bfast, combined):
        if own[tilingstats.STATSEL_COLTYPE] == tilingstats.STAT_DTYPE_INT:
            ic[comb[tilingstats.STATSEL_COLARRAYINDEX]] = bic[own[tilingstats.STATSEL_COLARRAYINDEX]]
        else:
            fc[comb[tilingstats.STATSEL_COLARRAYINDEX]] = bfc[own[tilingstats.STATSEL_COLARRAYINDEX]]


def calcPerSegmentStatsDistributedBands(engine, comm, hist, bandSelections, missingStatsValue=-9999,
                                        imgNullVal=None, info=None):
    """calcPerSegmentStatsDistributed for several bands in one call, as tilingstats.calcPerSegmentStatsTiledBands
    is to calcPerSegmentStatsTiled: ``bandSelections`` is a list of (imgbandnum, statsSelection); a band may be
    named by several entries, column names are unique over the call, ``imgNullVal`` is one value for all entries
    or a list with one per entry (None: no null value).  The columns lie in the order of the entries.  Bad
    arguments raise tilingstats.PyShepSegStatsError before any collective, alike on every rank.

    What depends on the labels alone happens once whatever the number of entries: the local histogram and the
    classification of every id against ``hist``, the straddlers' ids on the wire (each distinct band's values
    travel beside them, once), the pick of this rank's id share, and ONE all-reduce of all columns.  Under RCCL
    with a device engine nothing crosses the host (shp_dstats_local_bands_dev -> all-gather of the ids and of the
    values in the bands' pixel type -> shp_dstats_merge_bands_dev -> ncclAllReduce); the other transports carry
    the same arrays as raw bytes between the engine's host methods (_distributedStats).  One entry is no special
    route.  A ``hist`` that gives an id FEWER pixels than a rank holds of it raises on every rank.

    ``info`` (a dict, optional) receives 'straddlers' (segments) and 'straddler_pixels' of the whole job, 'path',
    'bands' (distinct bands read) and 'exchange_bytes' (the straddlers' ids and values all ranks put on the wire,
    without padding: on the device path straddler_pixels * (4 + bands * itemsize)).  Returns (intcols int64 (nInt,
    maxSegId+1), floatcols float32 (nFloat, maxSegId+1), statsSelection_fast) on every rank, every column
    bit-identical to the column calcPerSegmentStatsDistributed returns for its entry alone."""
    from . import tilingstats
    (fast, bandOfStat, nInt, nFloat) = tilingstats.makeBandStatsSelection(bandSelections)
    bandSelections = [(int(b), list(sel)) for (b, sel) in bandSelections]
    nullVals = tilingstats._entryNullVals(imgNullVal, len(bandSelections), [None] * len(bandSelections))
    nBands = _engineBandCount(engine)
    for (b, _sel) in bandSelections:
        if b < 1 or (nBands is not None and b > nBands):
            raise tilingstats.PyShepSegStatsError("band %d not in image" % b)
    return _distributedStats(engine, comm, hist, bandSelections, fast, bandOfStat, nInt, nFloat, nullVals,
                             missingStatsValue, info)


def _distributedStats(engine, comm, hist, bandSelections, fast, bandOfStat, nInt, nFloat, nullVals, missingStatsValue,
                      info):
    """What calcPerSegmentStatsDistributed and calcPerSegmentStatsDistributedBands share: the split over entries.
    bandSelections: a list of (imgbandnum, statsSelection), ``fast`` their combined fast selection, bandOfStat[i]
    the entry of statistic i, nullVals one null value (or None) per entry.

    What it calls on the engine, beside histogram(maxSegId) -- either set of methods will do:
      statsBandsOnDevice(comm, hist, planes, planeOfEntry, fast, perBand, nullVals, nInt, nFloat, missing) ->
          (ic, fc, straddlers, their pixels, bytes exchanged): the whole split on the device (deviceStatsBands);
          optional, and only asked of a communicator that is on the device.
      localStatsBands(bandNums, S, fast, perBand, nInt, nFloat, missing, nullVals) -> (ic, fc): all entries' columns
          over this rank's rows; gatherFlaggedBands(planes, S, flags, count) -> (ids, (len(planes), count) values):
          the pixels of the flagged ids, every distinct band's values in the order of the ids;
          statsOfPairsBands(segs, vals, K, planeOfEntry, fast, perBand, nInt, nFloat, missing, nullVals) -> (ic, fc):
          the entries' columns of a list of (compact id 1..K, values per distinct band) pairs.
      or, entry by entry, localStats(imgbandnum, S, fast, nInt, nFloat, missing, imgNullVal) -> (ic, fc),
          gatherFlagged(imgbandnum, S, flags, count) -> (ids, values) in any order, statsOfPairs(segs, vals, K,
          fast, nInt, nFloat, missing, imgNullVal) -> (ic, fc), each with the entry's own fast selection."""
    from . import tilingstats
    Err = tilingstats.PyShepSegStatsError
    nEntries = len(bandSelections)
    planes = tilingstats._planeNumbers(bandSelections)
    planeOfEntry = [planes.index(b) for (b, _sel) in bandSelections]
    perBand = numpy.ascontiguousarray([len(sel) for (_b, sel) in bandSelections], dtype=numpy.int32)
    if getattr(comm, 'onDevice', False) and hasattr(engine, 'statsBandsOnDevice'):
        (ic, fc, nStrad, nPix, nBytes) = engine.statsBandsOnDevice(comm, hist, planes, planeOfEntry, fast, perBand, nullVals,
                                                                  nInt, nFloat, missingStatsValue)
        if info is not None:
            info.update(straddlers=nStrad, straddler_pixels=nPix, path='device', bands=len(planes), exchange_bytes=nBytes)
        return ic, fc, fast
    ownFast = [tilingstats.makeFastStatsSelection(list(range(len(sel))), sel) for (_b, sel) in bandSelections]
    hist = numpy.asarray(hist).astype(numpy.int64)
    S = len(hist) - 1
    # ---- the labels' part, once: who is complete here, who straddles
    lh = numpy.asarray(engine.histogram(S)).astype(numpy.int64)
    lh[0] = 0
    nStale = int((lh[1:] > hist[1:]).sum())
    _raiseOnAllRanks(comm, None if nStale == 0 else Err(
        "%d segment ids have more pixels in this rank's rows than the histogram gives them in the whole raster: "
        "the histogram does not belong to these labels" % nStale))
    complete = (lh == hist) & (lh > 0)
    strad = (lh > 0) & (lh < hist)
    if hasattr(engine, 'localStatsBands'):
        (ic, fc) = engine.localStatsBands([b for (b, _sel) in bandSelections], S, fast, perBand, nInt, nFloat,
                                          missingStatsValue, nullVals)
    else:
        ic = numpy.zeros((nInt, S + 1), dtype=numpy.int64)
        fc = numpy.zeros((nFloat, S + 1), dtype=numpy.float32)
        for (k, (b, _sel)) in enumerate(bandSelections):
            (bfast, bInt, bFloat) = ownFast[k]
            (bic, bfc) = engine.localStats(b, S, bfast, bInt, bFloat, missingStatsValue, nullVals[k])
            _placeEntryColumns(ic, fc, bic, bfc, bfast, fast[bandOfStat == k])
    keep = complete.copy()
    if comm.rank == 0:
        keep |= (hist == 0)                 # ids nobody holds (and row 0): "missing" rows, once
    ic[:, ~keep] = 0
    fc[:, ~keep] = 0
    # ---- the straddlers' pixels: the ids once, one value array per distinct band
    flags = strad.astype(numpy.uint8)
    count = int(lh[strad].sum())
    if hasattr(engine, 'gatherFlaggedBands'):
        (pairIds, pairVals) = engine.gatherFlaggedBands(planes, S, flags, count)
        pairVals = [pairVals[p] for p in range(len(planes))]
    else:
        # gatherFlagged promises no order, so a plane's values are matched to the ids of ITS call: both sorted by id
        # (a segment's statistics do not depend on the order of its pixels)
        (pairIds, pairVals) = (None, [])
        for b in planes:
            (ids_b, vals_b) = engine.gatherFlagged(b, S, flags, count)
            order = numpy.argsort(ids_b, kind='stable')
            ids_b = numpy.asarray(ids_b)[order]
            if pairIds is None:
                pairIds = ids_b
            elif not numpy.array_equal(pairIds, ids_b):
                raise Err("internal: the straddlers' pixels of band %d are not those of band %d" % (b, planes[0]))
            pairVals.append(numpy.asarray(vals_b)[order])
    allPairs = comm.allgather_arrays([pairIds] + pairVals)
    segs = numpy.concatenate([p[0] for p in allPairs])
    vals = [numpy.concatenate([p[1 + k] for p in allPairs]) for k in range(len(planes))]
    nBytes = int(segs.nbytes + sum(v.nbytes for v in vals))
    # ---- this rank's share of the straddlers: picked once
    (lo, hi) = idRange(comm.rank, comm.world, S)
    mine = (segs >= lo) & (segs < hi)
    if mine.any():
        (ids, compact) = numpy.unique(segs[mine], return_inverse=True)
        seg1 = (compact + 1).astype(numpy.uint32)
        myVals = [numpy.ascontiguousarray(v[mine]) for v in vals]
        if hasattr(engine, 'statsOfPairsBands'):
            (ic2, fc2) = engine.statsOfPairsBands(seg1, myVals, len(ids), planeOfEntry, fast, perBand, nInt, nFloat,
                                                  missingStatsValue, nullVals)
        else:
            ic2 = numpy.zeros((nInt, len(ids) + 1), dtype=numpy.int64)
            fc2 = numpy.zeros((nFloat, len(ids) + 1), dtype=numpy.float32)
            for k in range(nEntries):
                (bfast, bInt, bFloat) = ownFast[k]
                (bic, bfc) = engine.statsOfPairs(seg1, myVals[planeOfEntry[k]], len(ids), bfast, bInt, bFloat,
                                                 missingStatsValue, nullVals[k])
                _placeEntryColumns(ic2, fc2, bic, bfc, bfast, fast[bandOfStat == k])
        ic[:, ids] = ic2[:, 1:]
        fc[:, ids] = fc2[:, 1:]
    if info is not None:
        info.update(straddlers=int(len(numpy.unique(segs))), straddler_pixels=int(len(segs)), path='host',
                    bands=len(planes), exchange_bytes=nBytes)
    if comm.world > 1:
        # one all-reduce: the integer columns and the float columns' bit patterns side by side
        block = numpy.concatenate([ic.reshape(-1), fc.view(numpy.int32).reshape(-1).astype(numpy.int64)])
        block = comm.allreduce_sum_i64(block)
        ic = block[:ic.size].reshape(nInt, S + 1)
        fc = block[ic.size:].astype(numpy.int32).view(numpy.float32).reshape(nFloat, S + 1)
    return ic, fc, fast


def deviceStatsBands(c, comm, d_seg, d_bands, dtypeCode, nRows, nCols, hist, fast, perBand, hasNull, nullVals, nInt,
                     nFloat, missing, fetch=True):
    """The device-resident data path of calcPerSegmentStatsDistributed[Bands] for ONE rank, over entries: label
    rows d_seg (nRows x nCols uint32) in the HBM of context ``c``; comm: allgather_obj (control data only),
    allgather_dev, allreduce_dev_i64.  d_bands: one device address per entry (this rank's rows of
    the entry's band; entries that read the same band give the same address, and the distinct addresses must
    number alike on every rank -- a rank without rows (nRows 0) passes distinct made-up ones, which are not read,
    and may pass dtypeCode None: it learns the pixel type from the other ranks);
    perBand / hasNull / nullVals: statistics, null flag and null value per entry; ``fast`` the combined selection.
    ``hist``: the global histogram, a numpy array or ('dev', address, length) when it is in device memory already.
    fetch=False: the assembled columns are not copied to the host (ic = fc = None).  Two all-gathers (the ids; the
    values, every rank's block = one row per distinct band, the same stride on every rank) and one all-reduce.  A
    histogram that cannot belong to these labels (shp_dstats_local_bands_dev) raises _lib.ShepsegHipError on every
    rank.  Returns (ic, fc, straddling segments, their pixels, payload bytes of the all-gathers over all ranks)."""
    L = c._L
    planes = list(dict.fromkeys(int(p) for p in d_bands))
    nPlanes = len(planes)
    d_planes = (ctypes.c_void_p * nPlanes)(*planes)
    planeOfBand = numpy.ascontiguousarray([planes.index(int(p)) for p in d_bands], dtype=numpy.int32)
    nBandsIn = len(planeOfBand)
    fast = numpy.ascontiguousarray(fast, dtype=numpy.uint32)
    perBand = numpy.ascontiguousarray(perBand, dtype=numpy.int32)
    hasNull = numpy.ascontiguousarray(hasNull, dtype=numpy.int32)
    nullVals = numpy.ascontiguousarray(nullVals, dtype=numpy.int64)
    with distdev.Scratch(c) as s:
        (d_hist, ns, _h32) = distdev.residentHist(s, c, hist)
        S = ns - 1
        colWords = distdev.colWords(nInt, nFloat, ns)
        d_cols = distdev.allocColumns(s, c, colWords)
        (pSeg, pVal) = (ctypes.c_void_p(), ctypes.c_void_p())
        (nPairs, nStrad, rowBytes) = (ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0))
        err = None
        try:
            c.check(L.shp_dstats_local_bands_dev(c.handle, ctypes.c_void_p(d_seg), d_planes, nPlanes, _lib.ptr(planeOfBand),
                                                 dtypeCode or 0, nBandsIn, nRows, nCols, S, _lib.ptr(hasNull),
                                                 _lib.ptr(nullVals), _lib.ptr(fast), _lib.ptr(perBand), int(missing), d_hist,
                                                 int(comm.rank == 0), d_cols, ctypes.byref(pSeg), ctypes.byref(pVal),
                                                 ctypes.byref(rowBytes), ctypes.byref(nPairs), ctypes.byref(nStrad)))
        except _lib.ShepsegHipError as e:      # (raised below, on every rank: the pair counts carry it)
            err = e
        got = comm.allgather_obj((None if err is None else (type(err).__name__, str(err)), int(nPairs.value),
                                  dtypeCode))                                          # control data
        _raiseFirstError(comm, err, [g[0] for g in got])
        if dtypeCode is None:
            dtypeCode = ([g[2] for g in got if g[2] is not None] or [0])[0]
        itemsize = [dt for (dt, code) in _lib.SHP_DTYPES.items() if code == dtypeCode][0].itemsize
        counts = [int(g[1]) for g in got]
        (merged, nIds) = (ctypes.c_int64(0), ctypes.c_int64(0))
        # ---- the straddlers' pixels of all ranks: the ids, then one row of values per distinct band
        (d_allS, slot) = distdev.gatherRecords(s, c, comm, pSeg, nPairs.value, counts, 4)
        if slot > 0:
            slotRow = (slot * itemsize + 15) // 16 * 16       # a plane's row of a rank's block: the same on every rank
            d_sendV = s.alloc(nPlanes * slotRow)
            d_allV = s.alloc(comm.world * nPlanes * slotRow)
            for p in range(nPlanes if nPairs.value else 0):
                c.check(L.shp_dev_copy(c.handle, ctypes.c_void_p(d_sendV.value + p * slotRow),
                                       ctypes.c_void_p(pVal.value + p * rowBytes.value), nPairs.value * itemsize))
            comm.allgather_dev(d_sendV.value, d_allV.value, nPlanes * slotRow)
            (lo, hi) = idRange(comm.rank, comm.world, S)
            cnts = numpy.array(counts, dtype=numpy.uint32)
            c.check(L.shp_dstats_merge_bands_dev(c.handle, d_allS, d_allV, slot, slotRow, comm.world, _lib.ptr(cnts),
                                                 dtypeCode, nBandsIn, nPlanes, _lib.ptr(planeOfBand), S, _lib.ptr(hasNull),
                                                 _lib.ptr(nullVals), _lib.ptr(fast), _lib.ptr(perBand), int(missing), lo, hi,
                                                 d_cols, ctypes.byref(merged), ctypes.byref(nIds)))
        if comm.world > 1:
            comm.allreduce_dev_i64(d_cols.value, colWords)
        (ic, fc) = distdev.fetchColumns(c, d_cols, nInt, nFloat, ns, fetch)
    # the job's figures: the ranks' id shares partition the straddlers, the ranks' rows their pixels
    tot = comm.allgather_obj((int(nIds.value), int(nPairs.value)))
    nPix = int(sum(t[1] for t in tot))
    return ic, fc, int(sum(t[0] for t in tot)), nPix, nPix * (4 + nPlanes * itemsize)


def statsColumnsByName(bandSelections, intcols, floatcols, fast):
    """What calcPerSegmentStatsDistributedBands(engine, comm, hist, bandSelections, ...) returned, under the
    column names of ``bandSelections``: {name: 1-D array with one row per segment id} (rows of intcols / floatcols,
    not copies), the ``columns`` of writeColorTableFromRatColumnsDistributed.  One (imgbandnum, statsSelection)
    entry with calcPerSegmentStatsDistributed's result works alike."""
    from . import tilingstats
    names = [sel[0] for (_b, statsSelection) in bandSelections for sel in statsSelection]
    if len(names) != len(fast):
        raise tilingstats.PyShepSegStatsError("%d column names for a selection of %d statistics" % (len(names), len(fast)))
    out = {}
    for (name, row) in zip(names, fast):
        src = intcols if int(row[tilingstats.STATSEL_COLTYPE]) == tilingstats.STAT_DTYPE_INT else floatcols
        out[name] = src[int(row[tilingstats.STATSEL_COLARRAYINDEX])]
    return out
