"""The segment-neighbour table of the row-sharded multi-rank output, sharded by id (deviceNeighbours,
csrc/dneighbours.h), its reductions, and touching segments merged on it (deviceMerge, csrc/dnbrmerge.h)."""
import ctypes
import time

import numpy

from . import _lib
from . import distdev
from .distdev import idRange, spatialHaloPlan, disjointRowsError, _rowsCoverError, _writeRows


def deviceNeighbours(c, comm, d_seg, nRows, nCols, rowRange, maxSegId, fourConnected=True, fetch=True, info=None):
    """The device-resident data path of findSegmentNeighboursDistributed for ONE rank: output rows rowRange =
    (outLo, outHi) of an nRows x nCols label raster (nRows None: the largest outHi of the ranks) at d_seg (uint32)
    in the HBM of context ``c``; comm: allgather_obj, allgather_dev, allreduce_dev_i64.  maxSegId bounds the labels
    (DistResult.maxSegId) and is the table's last row.

    Every rank counts the pairs whose upper pixel lies in its rows, reading one halo row below them (the first row
    of the next rank that holds rows: spatialHaloPlan, one all-gather of a row per rank), and reduces them to its
    distinct pairs (shp_dnbr_local_dev).  Pairs with both ids in the rank's own id share (idRange) stay home; the
    others travel in one all-gather of 16-byte records, slot = the largest count of the ranks.  Every rank then
    picks the records with an id in its share, adds its home records and builds the CSR rows of its share
    (shp_dnbr_merge_dev); one integer all-reduce completes the numNeighbours / borderLength columns.  Control data
    travels first, so every error that depends on a rank's data is raised on every rank: a label above maxSegId
    (the message names the largest over all ranks), output rows shared by several ranks (SHEPSEG_SHARD=tiles).

    Returns a neighbours.SegmentNeighboursShare whose table stays in the context for reduceOverNeighboursDistributed
    (fetch=False: its arrays and columns are None, nothing is copied to the host).  ``info`` (a dict, optional)
    receives 'halo_rows' (of all ranks), 'records_local' (this rank's distinct pairs), 'records_home',
    'records_sent', 'records_picked' (taken from the gathered blocks, this rank's own among them), 'exchange_bytes'
    (16 x the records sent by all ranks + 4 nCols x the ranks that sent a halo row: what every rank receives) and
    'entries' (of this share)."""
    from . import neighbours
    Err = neighbours.PyShepSegNeighboursError
    t0 = time.perf_counter()
    err = None
    try:
        if int(maxSegId) != maxSegId or maxSegId < 0 or maxSegId >= 0xFFFFFFFE:
            err = "maxSegId must be an integer in 0..2^32 - 3 (got {})".format(maxSegId)
    except (TypeError, ValueError):
        err = "maxSegId must be an integer (got {!r})".format(maxSegId)
    ctrl = comm.allgather_obj((int(rowRange[0]), int(rowRange[1]), err, None if err else int(maxSegId), int(nCols),
                               bool(fourConnected)))                                          # control data
    distdev.raiseFirst(Err, [x[2] for x in ctrl])
    if len({x[3:] for x in ctrl}) != 1:
        raise Err("the ranks pass different maxSegId, columns or connectivity: %s" % sorted({x[3:] for x in ctrl}))
    (S, nCols) = (int(maxSegId), int(nCols))
    ranges = [(x[0], x[1]) for x in ctrl]
    nRows = distdev.allRows(ranges, nRows)
    distdev.raiseFirst(Err, [disjointRowsError(ranges, 'findSegmentNeighboursDistributed') or
                             _rowsCoverError(ranges, nRows)])
    plan = spatialHaloPlan(ranges, comm.rank, nRows, 0, 1)
    (lo, hi) = ranges[comm.rank]
    h = max(hi - lo, 0)
    (idLo, idHi) = idRange(comm.rank, comm.world, S)
    L = c._L
    timings = {}
    with distdev.Scratch(c) as s:
        # ---- the halo row: every rank's first row in one all-gather
        d_halo = None
        rowB = nCols * 4
        haloSenders = 0
        if comm.world > 1 and nCols > 0:
            d_send = s.alloc(rowB)
            d_rows = s.alloc(comm.world * rowB)
            if plan['send']:
                c.check(L.shp_dev_copy(c.handle, d_send, ctypes.c_void_p(d_seg), rowB))
            comm.allgather_dev(d_send.value, d_rows.value, rowB)
            haloSenders = sum(1 for (a, b) in ranges if b > a)
            if plan['recvBelow']:
                (_row, src, _slotRow, _n) = plan['recvBelow'][0]
                d_halo = ctypes.c_void_p(d_rows.value + src * rowB)
        timings['halo'] = time.perf_counter() - t0
        # ---- own rows: distinct pairs, home and travelling records
        t1 = time.perf_counter()
        (maxLabel, pTrav, ms) = (ctypes.c_uint32(0), ctypes.c_void_p(), ctypes.c_double(0))
        cnt = numpy.zeros(3, dtype=numpy.int64)
        c.check(L.shp_dnbr_local_dev(c.handle, ctypes.c_void_p(d_seg if h else None), h, nCols, d_halo if h else None, S,
                                     int(bool(fourConnected)), idLo, idHi, ctypes.byref(maxLabel), _lib.ptr(cnt),
                                     ctypes.byref(pTrav), ctypes.byref(ms)))
        got = comm.allgather_obj((int(maxLabel.value), int(cnt[2]), plan['below']))
        worst = max(g[0] for g in got)
        if worst > S:
            raise Err("segment id {} is above maxSegId {}".format(worst, S))
        timings['local'] = time.perf_counter() - t1
        # ---- the travelling records of all ranks
        t1 = time.perf_counter()
        counts = [g[1] for g in got]
        (d_all, slot) = distdev.gatherRecords(s, c, comm, pTrav, int(cnt[2]), counts, 16)
        timings['exchange'] = time.perf_counter() - t1
        # ---- the rows of this rank's id share
        t1 = time.perf_counter()
        ns = S + 1
        d_cols = s.alloc(2 * ns * 8)
        (picked, nent) = (ctypes.c_int64(0), ctypes.c_int64(0))
        cnts = numpy.array(counts, dtype=numpy.uint32)
        c.check(L.shp_dnbr_merge_dev(c.handle, d_all, slot, comm.world, _lib.ptr(cnts), d_cols, ctypes.byref(picked),
                                     ctypes.byref(nent), ctypes.byref(ms)))
        if comm.world > 1:
            comm.allreduce_dev_i64(d_cols.value, 2 * ns)
        timings['merge'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        (offsets, nbrs, lens, columns) = (None, None, None, None)
        if fetch:
            offsets = numpy.empty(idHi - idLo + 1, dtype=numpy.int64)
            nbrs = numpy.empty(nent.value, dtype=numpy.uint32)
            lens = numpy.empty(nent.value, dtype=numpy.int64)
            c.check(L.shp_dnbr_download(c.handle, _lib.ptr(offsets), _lib.ptr(nbrs), _lib.ptr(lens)))
            cols = numpy.empty((2, ns), dtype=numpy.int64)
            c.check(L.shp_dev_download(c.handle, _lib.ptr(cols), d_cols, cols.nbytes))
            columns = {'numNeighbours': cols[0].copy(), 'borderLength': cols[1].copy()}
        timings['download'] = time.perf_counter() - t1
    timings['total'] = time.perf_counter() - t0
    figures = dict(halo_rows=int(sum(g[2] for g in got)), records_local=int(cnt[0]), records_home=int(cnt[1]),
                   records_sent=int(cnt[2]), records_picked=int(picked.value),
                   exchange_bytes=16 * int(sum(counts)) + rowB * haloSenders, entries=int(nent.value))
    if info is not None:
        info.update(figures)
    share = neighbours.SegmentNeighboursShare((idLo, idHi), S, bool(fourConnected), offsets, nbrs, lens, columns,
                                              timings=timings, deviceMs=ms.value, info=figures)
    (share.residentSerial, share._residentCtx) = (_shareSerial(c), c.handle.value)
    return share


def _shareSerial(c):
    """the serial of the context's share table, None when it has none"""
    (serial, finished) = (ctypes.c_uint64(0), ctypes.c_int(0))
    c.check(c._L.shp_dnbr_table_serial(c.handle, ctypes.byref(serial), ctypes.byref(finished)))
    return serial.value if finished.value else None


def findSegmentNeighboursDistributed(engine, comm, dres, fourConnected=True, info=None):
    """neighbours.findSegmentNeighbours of the label raster that runDistributed(engine, comm, ...) /
    doTiledShepherdSegmentationDistributed(keepOutput=True) left sharded by rows over the ranks (a
    HipEngine(keepOutput=True); ``dres`` its DistResult), without gathering it.  The table comes back sharded by id:
    every rank gets a neighbours.SegmentNeighboursShare with the finished rows of the ids of its idRange, equal to
    those rows of the one-GPU table of the mosaic, and the complete numNeighbours / borderLength columns
    (deviceNeighbours).  A communicator that is not on the device carries the device buffers through the host
    (comm.HostStagedDev).  Output rows shared by several ranks (SHEPSEG_SHARD=tiles) are refused on every rank:
    run the segmentation with SHEPSEG_SHARD=rows.  ``info``: see deviceNeighbours."""
    from . import neighbours
    if not hasattr(engine, 'neighboursOnDevice'):
        raise neighbours.PyShepSegNeighboursError("the distributed neighbour table needs a device engine (HipEngine)")
    dcomm = distdev.deviceComm(comm, engine.c)
    return engine.neighboursOnDevice(dcomm, dres.maxSegId, fourConnected=fourConnected, info=info)


def _checkShare(share):
    """the rules a share table must keep before its ids index a column on the device"""
    from . import neighbours
    Err = neighbours.PyShepSegNeighboursError
    (lo, hi) = share.idRange
    off = numpy.asarray(share.offsets)
    if not (0 <= lo <= hi <= share.maxSegId + 1) or len(off) != hi - lo + 1:
        raise Err("the share's offsets do not have the length of its id range")
    if off[0] != 0 or off[-1] != len(share.neighbours) or (numpy.diff(off) < 0).any():
        raise Err("the share's offsets must run from 0 to the number of entries and not decrease")
    if len(share.neighbours) and int(numpy.max(share.neighbours)) > share.maxSegId:
        raise Err("the share names a neighbour above maxSegId {}".format(share.maxSegId))


def reduceOverNeighboursDistributed(engine, comm, share, columnSelections, ignoreValue=None, missingStatsValue=-9999):
    """neighbours.reduceOverNeighbours over the table findSegmentNeighboursDistributed left sharded by id: the same
    dictionary outName -> array of maxSegId + 1 rows, complete on every rank and bit for bit the one-GPU result.
    ``share``: this rank's neighbours.SegmentNeighboursShare; ``columnSelections`` as in reduceOverNeighbours, the
    FULL columns (maxSegId + 1 values, the same on every rank -- the statistics' columns are).  ``engine``: a
    HipEngine, or any object whose ``c`` is this rank's context.

    Every rank reduces the rows of its share (their neighbours' values come from the full column), each row in the
    summation order of csrc/nbrreduce.h, into full-length device columns that are 0 elsewhere; ONE integer
    all-reduce over all selected outputs assembles them (float64 as bit patterns: adding zeros is exact).  The
    arguments are checked by reduceOverNeighbours' rules before any collective; the column lengths and selections
    are then compared between the ranks and a difference raises on all of them.  A share table that is no longer on
    the device (another one was built or uploaded since) is uploaded again from the share's arrays."""
    from . import neighbours
    Err = neighbours.PyShepSegNeighboursError
    if not isinstance(share, neighbours.SegmentNeighboursShare) or share.offsets is None:
        raise Err("share must be a SegmentNeighboursShare with its arrays (findSegmentNeighboursDistributed)")
    (idLo, idHi) = share.idRange
    (plan, ignore, missing) = neighbours._checkReduceSelections(share, idHi - idLo, columnSelections, ignoreValue,
                                                                missingStatsValue)
    mine = (int(share.maxSegId), [(len(col), ctype, sorted({bit for (_n, bit, _d) in picked}))
                                  for (col, ctype, picked) in plan], ignore, missing)
    got = comm.allgather_obj(mine)
    if any(g != got[0] and not _sameReduceCall(g, got[0]) for g in got):
        raise Err("the ranks pass different columns or selections to reduceOverNeighboursDistributed "
                  "(column lengths %s)" % [[x[0] for x in g[1]] for g in got])
    t0 = time.perf_counter()
    c = engine.c
    L = c._L
    dcomm = distdev.deviceComm(comm, c)
    timings = {'upload': 0.0, 'uploaded': False, 'deviceMs': 0.0}
    _makeShareResident(c, share, timings)
    t1 = time.perf_counter()
    ns = share.maxSegId + 1
    bitsOf = [sorted({bit for (_n, bit, _d) in picked}) for (_col, _ctype, picked) in plan]
    nOut = sum(len(b) for b in bitsOf)
    with distdev.Scratch(c) as s:
        d_out = s.alloc(nOut * ns * 8)
        at = 0
        for ((column, ctype, _picked), bits) in zip(plan, bitsOf):
            mask = sum(1 << b for b in bits)
            ms = ctypes.c_double(0)
            c.check(L.shp_dnbr_reduce_dev(c.handle, _lib.ptr(column), ctype, ns, int(ignore is not None),
                                          0.0 if ignore is None else ignore, missing, mask,
                                          ctypes.c_void_p(d_out.value + at * ns * 8), ctypes.byref(ms)))
            timings['deviceMs'] += ms.value
            at += len(bits)
        if dcomm.world > 1:
            dcomm.allreduce_dev_i64(d_out.value, nOut * ns)
        block = numpy.empty((nOut, ns), dtype=numpy.int64)
        c.check(L.shp_dev_download(c.handle, _lib.ptr(block), d_out, block.nbytes))
    out = {}
    at = 0
    for ((_column, _ctype, picked), bits) in zip(plan, bitsOf):
        for (outName, bit, dtype) in picked:
            row = block[at + bits.index(bit)]
            out[outName] = row.view(dtype).copy()        # (outNames that ask for the same statistic get copies)
        at += len(bits)
    timings['reduce'] = time.perf_counter() - t1
    timings['total'] = time.perf_counter() - t0
    share.reduceTimings = timings
    return out


def _shareIsResident(c, share):
    serial = _shareSerial(c)
    return serial is not None and share.residentSerial == serial and share._residentCtx == c.handle.value


def _makeShareResident(c, share, timings):
    """``share`` becomes the context's share table unless it still is: its arrays are checked and uploaded.
    timings: 'upload' and 'uploaded' are brought up to date"""
    if _shareIsResident(c, share):
        return
    t0 = time.perf_counter()
    _checkShare(share)
    (idLo, idHi) = share.idRange
    offsets = numpy.ascontiguousarray(share.offsets, dtype=numpy.int64)
    nbrs = numpy.ascontiguousarray(share.neighbours, dtype=numpy.uint32)
    lens = numpy.ascontiguousarray(share.borderLengths, dtype=numpy.int64)
    (share.residentSerial, share._residentCtx) = (None, None)
    c.check(c._L.shp_dnbr_upload(c.handle, _lib.ptr(offsets), _lib.ptr(nbrs), _lib.ptr(lens), share.maxSegId, idLo, idHi,
                                 len(nbrs)))
    (share.residentSerial, share._residentCtx) = (_shareSerial(c), c.handle.value)
    timings['upload'] = time.perf_counter() - t0
    timings['uploaded'] = True


def _sameReduceCall(a, b):
    """two ranks' (maxSegId, [(length, type, bits)], ignore, missing) agree (NaN ignore values compare equal)"""
    def same(x, y):
        return x == y or (isinstance(x, float) and isinstance(y, float) and x != x and y != y)
    return a[0] == b[0] and a[1] == b[1] and same(a[2], b[2]) and same(a[3], b[3])


def gatherSegmentNeighbours(comm, share):
    """The whole table on every rank, as a neighbours.SegmentNeighbours, from the ranks' shares (host arrays through
    the communicator: for small tables and for tests).  offsets, neighbours and borderLengths equal
    neighbours.findSegmentNeighbours of the whole raster."""
    from . import neighbours
    mine = [numpy.asarray(share.idRange, dtype=numpy.int64), numpy.asarray(share.offsets, dtype=numpy.int64),
            numpy.asarray(share.neighbours, dtype=numpy.uint32), numpy.asarray(share.borderLengths, dtype=numpy.int64)]
    gather = getattr(comm, 'allgather_arrays', None) or comm.allgather_obj
    parts = sorted(gather(mine), key=lambda p: (int(p[0][0]), int(p[0][1])))
    S = share.maxSegId
    offsets = numpy.zeros(S + 2, dtype=numpy.int64)
    (at, base) = (0, 0)
    for (rng, off, _n, _l) in parts:
        (lo, hi) = (int(rng[0]), int(rng[1]))
        if lo != at or len(off) != hi - lo + 1:
            raise neighbours.PyShepSegNeighboursError("the ranks' shares do not partition the ids (share %d..%d after "
                                                      "id %d)" % (lo, hi, at))
        offsets[lo:hi + 1] = base + off
        (at, base) = (hi, base + int(off[-1]))
    if at != S + 1:
        raise neighbours.PyShepSegNeighboursError("the ranks' shares end at id %d, not at maxSegId %d" % (at - 1, S))
    nb = neighbours.SegmentNeighbours(offsets, numpy.concatenate([p[2] for p in parts]),
                                      numpy.concatenate([p[3] for p in parts]), S, share.fourConnected)
    return nb


# ---- touching segments merged on the id-sharded table (csrc/dnbrmerge.h) ---------------------------------------
def mergeRule(share, keyColumn=None, ignoreKey=None, minBorder=1, segSize=None, distanceColumns=None, maxDistance=None,
              mutualNearest=False, ignoreValue=None):
    """The link rule of a distributed merge over ``share``, checked by the rules of neighbours.mergeSegments
    (``distanceColumns`` None: ``keyColumn`` is required) or neighbours.mergeSimilarSegments, before any collective:
    what deviceMerge takes as ``rule``.  Columns are the full ones (share.maxSegId + 1 values)."""
    from . import neighbours
    if not isinstance(share, neighbours.SegmentNeighboursShare):
        raise neighbours.PyShepSegNeighboursError("share must be a SegmentNeighboursShare "
                                                  "(findSegmentNeighboursDistributed, or a distributed merge's .neighbours)")
    nrows = int(share.maxSegId) + 1
    (keys, ignoreK, minBorder, sizes, _raster) = neighbours._checkMergeColumns(
        nrows, keyColumn, ignoreKey, minBorder, segSize, None, None, keyOptional=distanceColumns is not None)
    rule = dict(keys=keys, ignoreKey=ignoreK, minBorder=minBorder, sizes=sizes, columns=None, ignoreValue=None, thr2=None,
                mutual=False)
    if distanceColumns is not None:
        (columns, ignoreV, thr2) = neighbours._checkSimilarRule(distanceColumns, nrows, maxDistance, mutualNearest,
                                                                ignoreValue)
        rule.update(columns=columns, ignoreValue=ignoreV, thr2=thr2, mutual=bool(mutualNearest))
    return rule


def _ruleSignature(rule):
    """what the ranks' rules must agree in (floats as their hexadecimal text: NaN compares equal to NaN)"""
    def text(x):
        return None if x is None else float(x).hex()
    return (None if rule['keys'] is None else len(rule['keys']), rule['ignoreKey'], rule['minBorder'],
            None if rule['sizes'] is None else len(rule['sizes']),
            None if rule['columns'] is None else [len(col) for col in rule['columns']], text(rule['ignoreValue']),
            text(rule['thr2']), rule['mutual'])


def deviceMerge(c, comm, share, rule, d_seg=None, nRows=None, nCols=0, rowRange=None, outfile=None, info=None):
    """The device-resident data path of mergeSegmentsDistributed / mergeSimilarSegmentsDistributed for ONE rank.
    ``share``: the rank's neighbours.SegmentNeighboursShare on context ``c`` (uploaded again when another table has
    displaced it); ``rule``: mergeRule(share, ...); comm: allgather_obj, allgather_dev, allreduce_dev_i64.  With
    ``rowRange`` = (outLo, outHi) the rank's rows of an nRows x nCols label raster at d_seg (uint32, the HBM of ``c``;
    nRows None: the largest outHi) are recoded into a second device buffer, and written to ``outfile`` (a .npy path
    every rank can write) when that is given.

    The rank hooks the links among the entries a < b of its rows into a forest over all ids (shp_dnbr_mrg_begin /
    shp_dnbr_mrg_hook; the mutual rule first completes ``best`` with one integer all-reduce of S + 1 values).  One pair
    (id, root) per id that is not its own root travels in one all-gather, slot = the largest count; the other ranks'
    pairs are hooked in and the groups numbered, the same on every rank (shp_dnbr_mrg_number).  The entries a < b
    between two groups become the rank's records, split against its share idRange(rank, world, M) of the new ids;
    the travelling ones are all-gathered and the new share table built as deviceNeighbours builds the first
    (shp_dnbr_mrg_records, shp_dnbr_merge_dev, one integer all-reduce of the two columns).  Lengths, dtypes and scalar
    parameters are compared over the ranks first; every error that depends on a rank's data is raised on every rank.

    Returns a neighbours.MergedSegmentsShare.  ``info`` (a dict, optional) receives this rank's 'links',
    'forest_pairs' (pairs sent), 'records_entries' (entries a < b between two groups), 'records_local' (distinct pairs
    among them), 'records_home', 'records_sent', 'records_picked', 'entries' (of the new share), 'exchange_bytes' (8 x
    the pairs of all ranks + 16 x the travelling records of all ranks, + 8 (S + 1) with the mutual rule: what every
    rank receives) and 'deviceMs' (per step)."""
    from . import neighbours
    Err = neighbours.PyShepSegNeighboursError
    t0 = time.perf_counter()
    L = c._L
    S = int(share.maxSegId)
    ns = S + 1
    hasRows = rowRange is not None
    err = None
    if share.offsets is None and not _shareIsResident(c, share):
        err = ("rank %d: the share has no arrays (fetch=False) and its table is no longer on the device: nothing to "
               "merge over" % comm.rank)
    elif outfile is not None and not hasRows:
        err = "outfile needs the label rows to recode"
    elif outfile is not None and not (isinstance(outfile, str) and outfile.endswith('.npy')):
        err = "outfile must be None or a .npy path"
    rows = (int(rowRange[0]), int(rowRange[1])) if hasRows else None
    ctrl = comm.allgather_obj((err, S, tuple(share.idRange), bool(share.fourConnected), _ruleSignature(rule), rows,
                               int(nCols) if hasRows else None, outfile))                      # control data
    distdev.raiseFirst(Err, [x[0] for x in ctrl])
    # (everything but the error, the id share and the rows themselves must agree)
    calls = {repr((x[1], x[3], x[4], x[5] is None, x[6], x[7])) for x in ctrl}
    if len(calls) != 1:
        raise Err("the ranks pass different tables, columns, parameters or rasters to the distributed merge: %s"
                  % sorted(calls))
    for (r, x) in enumerate(ctrl):
        if tuple(x[2]) != idRange(r, comm.world, S):
            raise Err("rank %d holds the ids %s, not its share %s of 0..%d" % (r, tuple(x[2]), idRange(r, comm.world, S), S))
    (lo, hi, h) = (0, 0, 0)
    if hasRows:
        ranges = [x[5] for x in ctrl]
        nRows = distdev.allRows(ranges, nRows)
        nCols = int(nCols)
        distdev.raiseFirst(Err, [disjointRowsError(ranges, 'the distributed merge') or _rowsCoverError(ranges, nRows)])
        (lo, hi) = ranges[comm.rank]
        h = max(hi - lo, 0)
    timings = {'upload': 0.0, 'uploaded': False}
    ms = {}
    nbOut = max(h * nCols * 4, 16)
    with distdev.Scratch(c) as s:
        _makeShareResident(c, share, timings)
        # ---- the links of this rank's rows, hooked; the mutual rule's best completed first
        t1 = time.perf_counter()
        (keys, sizes, columns) = (rule['keys'], rule['sizes'], rule['columns'])
        (ignoreK, ignoreV, thr2) = (rule['ignoreKey'], rule['ignoreValue'], rule['thr2'])
        cols = None if columns is None else (ctypes.c_void_p * len(columns))(*[col.ctypes.data for col in columns])
        (pBest, ms2) = (ctypes.c_void_p(), numpy.zeros(2, dtype=numpy.float64))
        c.check(L.shp_dnbr_mrg_begin(
            c.handle, cols, 0 if columns is None else len(columns), ns, int(ignoreV is not None),
            0.0 if ignoreV is None else ignoreV, int(thr2 is not None), 0.0 if thr2 is None else thr2, int(rule['mutual']),
            None if keys is None else _lib.ptr(keys), int(ignoreK is not None), 0 if ignoreK is None else ignoreK,
            rule['minBorder'], None if sizes is None else _lib.ptr(sizes), ctypes.byref(pBest), _lib.ptr(ms2)))
        if ms2[0]:
            ms['records'] = float(ms2[0])
        if rule['mutual']:
            ms['best'] = float(ms2[1])
            if comm.world > 1:
                comm.allreduce_dev_i64(pBest.value, ns)
        (cnt, pPairs) = (numpy.zeros(3, dtype=numpy.int64), ctypes.c_void_p())
        c.check(L.shp_dnbr_mrg_hook(c.handle, _lib.ptr(cnt), ctypes.byref(pPairs), _lib.ptr(ms2)))
        (ms['hook'], ms['pairs']) = (float(ms2[0]), float(ms2[1]))
        (links, nPairs) = (int(cnt[0]), int(cnt[2]))
        timings['hook'] = time.perf_counter() - t1
        # ---- the forests of all ranks, the groups
        t1 = time.perf_counter()
        got = comm.allgather_obj((nPairs, links))
        pairCounts = [g[0] for g in got]
        (d_all, slot) = distdev.gatherRecords(s, c, comm, pPairs, nPairs, pairCounts, 8, inPlaceAlone=True)
        (M, pHist) = (ctypes.c_uint32(0), ctypes.c_void_p())
        cnts = numpy.array(pairCounts, dtype=numpy.uint32)
        c.check(L.shp_dnbr_mrg_number(c.handle, d_all, slot, comm.world, _lib.ptr(cnts), comm.rank, ctypes.byref(M),
                                      ctypes.byref(pHist), _lib.ptr(ms2)))
        (ms['pairhook'], ms['renumber']) = (float(ms2[0]), float(ms2[1]))
        M = int(M.value)
        res = neighbours.MergedSegmentsShare()
        (res.groupsSerial, res._groupsCtx) = (neighbours._groupSerials(c)[0], c.handle.value)
        res.recode = numpy.empty(ns, dtype=numpy.uint32)
        res.representative = numpy.empty(M + 1, dtype=numpy.uint32)
        res.groupSize = numpy.empty(M + 1, dtype=numpy.int64)
        if sizes is not None:
            res.hist = numpy.empty(M + 1, dtype=numpy.int64)
        c.check(L.shp_nbr_merge_groups(c.handle, _lib.ptr(res.recode), _lib.ptr(res.representative), _lib.ptr(res.groupSize),
                                       None if res.hist is None else _lib.ptr(res.hist)))
        timings['groups'] = time.perf_counter() - t1
        # ---- this rank's rows of the raster
        ms['recode'] = 0.0
        if hasRows:
            t1 = time.perf_counter()
            d_out = s.alloc(nbOut)
            (bad, msr) = (ctypes.c_uint32(0), ctypes.c_double(0))
            if h * nCols:
                c.check(L.shp_nbr_merge_recode_dev(c.handle, ctypes.c_void_p(d_seg), h * nCols, d_out, int(sizes is None),
                                                   ctypes.byref(bad), ctypes.byref(msr)))
            ms['recode'] = msr.value
            worst = max(comm.allgather_obj(int(bad.value)))
            if worst:
                raise Err("segment id {} is above maxSegId {}".format(worst, S))
            if sizes is None:
                if comm.world > 1:
                    comm.allreduce_dev_i64(pHist.value, M + 1)
                res.hist = numpy.empty(M + 1, dtype=numpy.int64)
                c.check(L.shp_nbr_merge_groups(c.handle, None, None, None, _lib.ptr(res.hist)))
            timings['recode'] = time.perf_counter() - t1
        # ---- the contracted table, sharded by the new ids
        t1 = time.perf_counter()
        (newLo, newHi) = idRange(comm.rank, comm.world, M)
        (rc, pTrav, msc) = (numpy.zeros(5, dtype=numpy.int64), ctypes.c_void_p(), ctypes.c_double(0))
        c.check(L.shp_dnbr_mrg_records(c.handle, newLo, newHi, _lib.ptr(rc), ctypes.byref(pTrav), ctypes.byref(msc)))
        got2 = comm.allgather_obj((int(rc[3]), int(rc[0]), int(rc[4])))
        wide = sum(g[2] for g in got2)
        if wide:
            raise Err("{} border lengths of the table are outside 1 .. 2^32 - 1: the contraction's records hold "
                      "32-bit lengths".format(wide))
        (share.residentSerial, share._residentCtx) = (None, None)        # (the new share table takes its place)
        travCounts = [g[0] for g in got2]
        (d_allRec, slotRec) = distdev.gatherRecords(s, c, comm, pTrav, int(rc[3]), travCounts, 16, inPlaceAlone=True)
        d_cols = s.alloc(2 * (M + 1) * 8)
        (picked, nent) = (ctypes.c_int64(0), ctypes.c_int64(0))
        cnts = numpy.array(travCounts, dtype=numpy.uint32)
        c.check(L.shp_dnbr_merge_dev(c.handle, d_allRec, slotRec, comm.world, _lib.ptr(cnts), d_cols, ctypes.byref(picked),
                                     ctypes.byref(nent), ctypes.byref(msc)))
        ms['contract'] = msc.value
        if comm.world > 1:
            comm.allreduce_dev_i64(d_cols.value, 2 * (M + 1))
        offsets = numpy.empty(newHi - newLo + 1, dtype=numpy.int64)
        nbrs = numpy.empty(nent.value, dtype=numpy.uint32)
        lens = numpy.empty(nent.value, dtype=numpy.int64)
        c.check(L.shp_dnbr_download(c.handle, _lib.ptr(offsets), _lib.ptr(nbrs), _lib.ptr(lens)))
        block = numpy.empty((2, M + 1), dtype=numpy.int64)
        c.check(L.shp_dev_download(c.handle, _lib.ptr(block), d_cols, block.nbytes))
        timings['contract'] = time.perf_counter() - t1
        # ---- the recoded rows to the file
        if outfile is not None:
            t1 = time.perf_counter()
            out = numpy.empty((h, nCols), dtype=numpy.uint32)
            if out.size:
                c.check(L.shp_dev_download(c.handle, _lib.ptr(out), d_out, out.nbytes))
            _writeRows(comm, outfile, out, lo, (nRows, nCols))
            timings['write'] = time.perf_counter() - t1
        figures = dict(links=links, forest_pairs=nPairs, records_entries=int(rc[0]), records_local=int(rc[1]),
                       records_home=int(rc[2]), records_sent=int(rc[3]), records_picked=int(picked.value),
                       entries=int(nent.value),
                       exchange_bytes=8 * sum(pairCounts) + 16 * sum(travCounts) + (8 * ns if rule['mutual'] else 0),
                       deviceMs=dict(ms))
        nshare = neighbours.SegmentNeighboursShare(
            (newLo, newHi), M, share.fourConnected, offsets, nbrs, lens,
            {'numNeighbours': block[0].copy(), 'borderLength': block[1].copy()}, deviceMs=msc.value, info=figures)
        (nshare.residentSerial, nshare._residentCtx) = (_shareSerial(c), c.handle.value)
        res.neighbours = nshare
        res.maxSegId = M
        res.links = sum(g[1] for g in got)
        res.recordsSorted = sum(g[1] for g in got2)
        res.stepDeviceMs = ms
        res.deviceMs = sum(ms.values())
        res.info = figures
        if hasRows:
            res.rowRange = (lo, hi)
            if h:
                res.outDev = (s.keep(d_out).value, h, nCols, nbOut)
    timings['total'] = time.perf_counter() - t0
    res.timings = timings
    if info is not None:
        info.update(figures)
    return res


def _mergeDistributed(engine, comm, share, rule, dres, outfile, info):
    from . import neighbours
    Err = neighbours.PyShepSegNeighboursError
    if outfile is not None and not (isinstance(outfile, str) and outfile.endswith('.npy')):
        raise Err("outfile must be None or a .npy path")
    if outfile is not None and dres is None:
        raise Err("outfile needs dres: the rows to recode are the engine's kept output")
    dcomm = distdev.deviceComm(comm, engine.c)
    if dres is None:
        return deviceMerge(engine.c, dcomm, share, rule, info=info)
    if not hasattr(engine, 'mergeOnDevice'):
        raise Err("recoding the kept output needs a device engine (HipEngine)")
    return engine.mergeOnDevice(dcomm, share, rule, dres.nRows, outfile=outfile, info=info)


def mergeSegmentsDistributed(engine, comm, share, keyColumn, ignoreKey=None, minBorder=1, segSize=None, dres=None,
                             outfile=None, info=None):
    """neighbours.mergeSegments over the table findSegmentNeighboursDistributed left sharded by id, without gathering
    it: every rank gets a neighbours.MergedSegmentsShare whose ``recode``, ``representative``, ``groupSize``, ``hist``,
    ``maxSegId``, ``links`` and ``recordsSorted`` are complete and equal the one-GPU function's on the whole table, and
    whose ``neighbours`` is the rank's share idRange(rank, world, maxSegId) of the contracted table -- resident on the
    rank's context, so reduceOverNeighboursDistributed uploads nothing and the next round's merge takes it as
    ``share``.  ``share``: this rank's SegmentNeighboursShare; ``keyColumn``, ``ignoreKey``, ``minBorder`` and
    ``segSize`` as in mergeSegments, the FULL columns, the same on every rank.  ``engine``: a HipEngine, or any object
    whose ``c`` is this rank's context.

    ``dres`` (the DistResult of the run whose output the engine has kept): the rank's output rows are recoded into a
    second device buffer, ``result.outDev`` with ``result.rowRange``; without ``segSize`` the new ``hist`` is counted
    in that pass.  ``outfile`` (a .npy path every rank can write) also receives them: rank 0 creates the file, every
    rank writes its rows.  A label above ``share.maxSegId`` raises on every rank with the largest such label.  Output
    rows shared by several ranks (SHEPSEG_SHARD=tiles) are refused on every rank.  ``info``: see deviceMerge."""
    return _mergeDistributed(engine, comm, share, mergeRule(share, keyColumn, ignoreKey, minBorder, segSize), dres,
                             outfile, info)


def mergeSimilarSegmentsDistributed(engine, comm, share, distanceColumns, maxDistance=None, mutualNearest=False,
                                    ignoreValue=None, keyColumn=None, ignoreKey=None, minBorder=1, segSize=None,
                                    dres=None, outfile=None, info=None):
    """neighbours.mergeSimilarSegments over the id-sharded table: mergeSegmentsDistributed with the link rule of
    mergeSimilarSegments (``distanceColumns``, ``maxDistance``, ``mutualNearest``, ``ignoreValue``, optional
    ``keyColumn``), bit for bit the one-GPU groups.  With ``mutualNearest`` every rank finds the best neighbour of the
    rows of its share and one integer all-reduce of maxSegId + 1 values hands every rank all of them."""
    if distanceColumns is None:
        from . import neighbours
        raise neighbours.PyShepSegNeighboursError("distanceColumns must be a list of 1-D columns")
    rule = mergeRule(share, keyColumn, ignoreKey, minBorder, segSize, distanceColumns, maxDistance, mutualNearest,
                     ignoreValue)
    return _mergeDistributed(engine, comm, share, rule, dres, outfile, info)


def aggregateToGroupsDistributed(engine, merged, columnSelections, weights=None, ignoreValue=None, missingStatsValue=-9999):
    """neighbours.aggregateToGroups on this rank's context: the same dictionary on every rank, bit for bit the
    one-GPU result (a group's sums run in the order of its member list, wherever they run).  Every rank reduces ALL
    groups from the full columns and no collective is involved: the groups are on every rank's context after the
    merge, and the reduction costs less than sending its result would."""
    from . import neighbours
    return neighbours._aggregateOnContext(engine.c, merged, columnSelections, weights, ignoreValue, missingStatsValue)
