"""Per-segment neighbour lists and border lengths of a label raster.

The reference stops at statistics that describe a segment by itself; an object-based workflow next asks
which segments touch which, and along how much border (neighbour context for a classification, "relative
border to", merge candidates, colouring the segments like a map).  ``findSegmentNeighbours`` answers that
from the label raster alone, on the GPU (csrc/neighbours.h), as a CSR table over the segment ids.

Definition, all integers: two pixels are adjacent when one is the E or S neighbour of the other, and with
``fourConnected=False`` the SE and SW neighbour as well.  Every adjacent pixel pair with labels ``a != b``,
both non-zero, adds 1 to the border length of ``(a, b)`` and of ``(b, a)``.  Label 0 is no segment: it has
no neighbours and is nobody's neighbour.  Ids without pixels have empty rows.

On the row-sharded output of a multi-rank run the same table is built without gathering the labels, sharded by
segment id (distributed.findSegmentNeighboursDistributed -> SegmentNeighboursShare, csrc/dneighbours.h), and columns
are reduced over it there (distributed.reduceOverNeighboursDistributed).

``reduceOverNeighbours`` computes per-segment columns over the table's rows; ``mergeSegments`` acts on a merge
candidate: under a column of class codes, touching segments of one class become one object -- new ids, the recoded
raster and the table of the merged objects (csrc/nbrmerge.h).  ``mergeSimilarSegments`` merges by a distance between
per-segment columns instead, and ``aggregateToGroups`` carries columns of the old segments to the merged objects
(csrc/nbragg.h): table -> merge -> columns of the groups -> reductions over the contracted table -> merge again, all on
the device.

There is no CPU fallback: without a GPU the call fails as every entry point of this package does.
"""
import ctypes
import time

import numpy

from . import _lib
from . import labelsource
from . import tiling


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
        self.residentSerial = None
        self._residentCtx = None
        self.reduceTimings = {}

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


class SegmentNeighboursShare(object):
    """One rank's part of the table of distributed.findSegmentNeighboursDistributed: the finished rows of the ids
    ``idRange`` = (idLo, idHi) (distributed.idRange), which are the rows idLo .. idHi - 1 of the one-GPU table of
    the whole raster.

    ``offsets``: int64, ``idHi - idLo + 1`` row boundaries from 0 (row i is id ``idLo + i``); ``neighbours``:
    uint32 ids, ascending within a row; ``borderLengths``: int64.  ``columns``: {'numNeighbours', 'borderLength'}
    of ALL ids, complete on every rank: the arrays SegmentNeighbours.columns gives.  ``timings``: seconds per step;
    ``deviceMs``: GPU time of this rank's kernels.  ``info``: the figures of the exchange
    (distributed.deviceNeighbours)."""
    def __init__(self, idRange, maxSegId, fourConnected, offsets, neighbours, borderLengths, columns, timings=None,
                 deviceMs=None, info=None):
        self.idRange = (int(idRange[0]), int(idRange[1]))
        self.maxSegId = int(maxSegId)
        self.fourConnected = bool(fourConnected)
        self.offsets = offsets
        self.neighbours = neighbours
        self.borderLengths = borderLengths
        self.columns = columns
        self.timings = timings if timings is not None else {}
        self.deviceMs = deviceMs
        self.info = info if info is not None else {}
        self.residentSerial = None
        self._residentCtx = None
        self.reduceTimings = {}

    def neighboursOf(self, segId):
        """(ids, lengths) of one segment of the share: views of ``neighbours`` and ``borderLengths``"""
        segId = int(segId)
        (lo, hi) = self.idRange
        if segId < lo or segId >= hi:
            raise PyShepSegNeighboursError("segment id {} is outside this rank's share {}..{}".format(segId, lo, hi - 1))
        (a, b) = (int(self.offsets[segId - lo]), int(self.offsets[segId - lo + 1]))
        return (self.neighbours[a:b], self.borderLengths[a:b])


def _checkArgs(segfile, maxSegId):
    """the labelsource.Labels of the raster: everything that can be refused before the GPU is touched"""
    return labelsource.resolve(segfile, maxSegId, PyShepSegNeighboursError)


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
    labels = _checkArgs(segfile, maxSegId)
    t0 = time.perf_counter()
    c = _lib.ctx()
    L = c._L
    timings = {}
    with labelsource.LabelSource(c, labels) as src:
        c.check(L.shp_nbr_begin(c.handle, -1 if labels.maxSegId is None else labels.maxSegId, int(bool(fourConnected))))
        for (y0, y1, dseg, _above, more) in src.blocks(chunkPixels, below=True):
            c.check(L.shp_nbr_accumulate_dev(c.handle, dseg, y1 - y0, labels.ncols, int(more)))
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
        serial = _tableSerial(c)
    timings['total'] = time.perf_counter() - t0
    nb = SegmentNeighbours(offsets, nbrs, lens, S.value, bool(fourConnected), pairsSeen=int(counters[0]),
                           recordsSorted=int(counters[1]), timings=timings, deviceMs=ms.value,
                           blocksRerun=int(counters[2]))
    (nb.residentSerial, nb._residentCtx) = (serial, c.handle.value)
    return nb


# ---- columns reduced over the table (csrc/nbrreduce.h) ---------------------------------------------------------
# statName -> (bit of the C call's mask, dtype of the column)
REDUCE_STATS = {'count': (0, numpy.int64), 'border': (1, numpy.int64), 'min': (2, numpy.float64),
                'max': (3, numpy.float64), 'mean': (4, numpy.float64), 'bordermean': (5, numpy.float64),
                'meanabsdiff': (6, numpy.float64), 'bordertohigher': (7, numpy.int64), 'nearest': (8, numpy.int64)}
_COLUMN_TYPES = {numpy.dtype(numpy.float64): 0, numpy.dtype(numpy.float32): 1, numpy.dtype(numpy.int64): 2}


def _tableSerial(c):
    """the serial of the context's finished table, None when it has none"""
    (serial, finished) = (ctypes.c_uint64(0), ctypes.c_int(0))
    c.check(c._L.shp_nbr_table_serial(c.handle, ctypes.byref(serial), ctypes.byref(finished)))
    return serial.value if finished.value else None


def residentTableSerial():
    """The serial of the neighbour table the calling thread's context holds on the device, None without one.
    Every table built or uploaded in the process has a serial of its own."""
    return _tableSerial(_lib.ctx())


def _makeResident(c, nb, timings):
    """``nb`` becomes the context's finished table unless it still is: then, and for a table built by hand, the three
    arrays are uploaded and checked on the device.  timings: 'upload', 'uploaded' and 'deviceMs' are brought up to date"""
    t0 = time.perf_counter()
    L = c._L
    serial = _tableSerial(c)
    if serial is None or nb.residentSerial != serial or nb._residentCtx != c.handle.value:
        offsets = numpy.ascontiguousarray(nb.offsets, dtype=numpy.int64)
        nbrs = numpy.ascontiguousarray(nb.neighbours, dtype=numpy.uint32)
        lens = numpy.ascontiguousarray(nb.borderLengths, dtype=numpy.int64)
        ms = ctypes.c_double(0)
        (nb.residentSerial, nb._residentCtx) = (None, None)
        rc = L.shp_nbr_upload(c.handle, _lib.ptr(offsets), _lib.ptr(nbrs), _lib.ptr(lens), int(nb.maxSegId), len(nbrs),
                              ctypes.byref(ms))
        if rc != 0:
            raise PyShepSegNeighboursError((L.shp_last_error(c.handle) or b'').decode())
        (nb.residentSerial, nb._residentCtx) = (_tableSerial(c), c.handle.value)
        timings['upload'] = time.perf_counter() - t0
        timings['uploaded'] = True
        timings['deviceMs'] += ms.value


def _number(value, name):
    return labelsource.number(value, name, PyShepSegNeighboursError)


def _checkReduceArgs(nb, columnSelections, ignoreValue, missingStatsValue):
    """([(contiguous column, type code, [(outName, bit, dtype), ...]), ...], ignore or None, missing): everything
    that can be refused before the GPU is touched"""
    if not isinstance(nb, SegmentNeighbours):
        raise PyShepSegNeighboursError("nb must be a SegmentNeighbours")
    return _checkReduceSelections(nb, int(nb.maxSegId) + 1, columnSelections, ignoreValue, missingStatsValue)


def _checkReduceSelections(nb, tableRows, columnSelections, ignoreValue, missingStatsValue):
    """_checkReduceArgs for a table ``nb`` of ``tableRows`` rows whose columns have maxSegId + 1 values (the whole
    table, or a SegmentNeighboursShare)"""
    nrows = int(nb.maxSegId) + 1
    if len(nb.offsets) != tableRows + 1 or len(nb.neighbours) != len(nb.borderLengths):
        raise PyShepSegNeighboursError("the table's arrays do not have the lengths of maxSegId {}".format(nb.maxSegId))
    return _planSelections(nrows, columnSelections, ignoreValue, missingStatsValue, REDUCE_STATS, _COLUMN_TYPES.get)


def _planSelections(nrows, columnSelections, ignoreValue, missingStatsValue, statTable, typeOf):
    """the plan of _checkReduceArgs for columns of ``nrows`` values: the statistics' names from ``statTable``, a
    dtype's type code from ``typeOf`` (None: not accepted)"""
    missing = _number(missingStatsValue, 'missingStatsValue')
    ignore = None if ignoreValue is None else _number(ignoreValue, 'ignoreValue')
    try:
        selections = [(column, list(stats)) for (column, stats) in columnSelections]
    except (TypeError, ValueError):
        raise PyShepSegNeighboursError("columnSelections must be a list of (column, [(outName, statName), ...])")
    if not selections:
        raise PyShepSegNeighboursError("columnSelections is empty")
    seen = set()
    plan = []
    for (i, (column, stats)) in enumerate(selections):
        if not isinstance(column, numpy.ndarray) or column.ndim != 1:
            raise PyShepSegNeighboursError("column {} must be a 1-D numpy array".format(i))
        if typeOf(column.dtype) is None:
            raise PyShepSegNeighboursError("column {} has dtype {}: float64, float32 or int64 wanted".format(
                i, column.dtype))
        if len(column) != nrows:
            raise PyShepSegNeighboursError("column {} has {} rows, the table maxSegId + 1 = {}".format(
                i, len(column), nrows))
        if not stats:
            raise PyShepSegNeighboursError("column {} has an empty selection".format(i))
        picked = []
        for item in stats:
            try:
                (outName, statName) = item
            except (TypeError, ValueError):
                raise PyShepSegNeighboursError("a selection must be (outName, statName) (got {!r})".format(item))
            if statName not in statTable:
                raise PyShepSegNeighboursError("unknown statName {!r}: one of {} wanted".format(
                    statName, ', '.join(sorted(statTable))))
            if outName in seen:
                raise PyShepSegNeighboursError("outName {!r} appears twice".format(outName))
            seen.add(outName)
            picked.append((outName,) + statTable[statName])
        plan.append((numpy.ascontiguousarray(column), typeOf(column.dtype), picked))
    return (plan, ignore, missing)


def reduceOverNeighbours(nb, columnSelections, ignoreValue=None, missingStatsValue=-9999):
    """
    Per-segment columns reduced over each segment's neighbours, on the GPU: a dictionary outName -> numpy array of
    ``maxSegId + 1`` rows, which merges into the statistics' column dictionaries as ``nb.columns`` does.

    ``nb`` is a SegmentNeighbours, from findSegmentNeighbours (its table is still on the device unless another one
    was built since: then, and for a table built by hand, the three arrays are uploaded and checked there).
    ``columnSelections``: a list of ``(column, [(outName, statName), ...])``; a column is a 1-D float64, float32 or
    int64 array of ``maxSegId + 1`` values and is widened to float64.

    With v the column, n the neighbour ids of a row r and w their border lengths, over the neighbours whose value
    is not ignored (NaN, or equal to ``ignoreValue``): ``count`` of them and ``border`` = sum w (int64); ``min``,
    ``max``, ``mean`` of v[n]; ``bordermean`` = sum(w v[n]) / sum w; and against the row's own value v[r]:
    ``meanabsdiff`` = sum(w |v[n] - v[r]|) / sum w, ``bordertohigher`` = sum of w where v[n] > v[r] (int64),
    ``nearest`` = the id with the smallest |v[n] - v[r]|, ties to the smallest id (int64).  A float statistic
    without a value (no neighbour left; an ignored v[r] for meanabsdiff) is ``missingStatsValue``, an integer one
    0.  The float sums are float64 in an order that depends on the row's length alone (csrc/nbrreduce.h), so a
    row's result does not depend on the rest of the table or on where the table came from.
    """
    (plan, ignore, missing) = _checkReduceArgs(nb, columnSelections, ignoreValue, missingStatsValue)
    t0 = time.perf_counter()
    c = _lib.ctx()
    L = c._L
    timings = {'upload': 0.0, 'uploaded': False, 'deviceMs': 0.0}
    _makeResident(c, nb, timings)
    t1 = time.perf_counter()
    out = {}
    nrows = int(nb.maxSegId) + 1
    for (column, ctype, picked) in plan:
        # one run per distinct statistic of the column; outNames that ask for the same one share it
        arrays = {}
        mask = 0
        ptrs = (ctypes.c_void_p * len(REDUCE_STATS))()
        for (_outName, bit, dtype) in picked:
            if bit not in arrays:
                arrays[bit] = numpy.empty(nrows, dtype=dtype)
                ptrs[bit] = arrays[bit].ctypes.data
                mask |= 1 << bit
        ms = ctypes.c_double(0)
        c.check(L.shp_nbr_reduce(c.handle, _lib.ptr(column), ctype, nrows, int(ignore is not None),
                                 0.0 if ignore is None else ignore, missing, mask, ptrs, ctypes.byref(ms)))
        timings['deviceMs'] += ms.value
        first = set()
        for (outName, bit, _dtype) in picked:
            out[outName] = arrays[bit] if bit not in first else arrays[bit].copy()
            first.add(bit)
    timings['reduce'] = time.perf_counter() - t1
    timings['total'] = time.perf_counter() - t0
    nb.reduceTimings = timings
    return out


# ---- touching segments of one class merged into one (csrc/nbrmerge.h) ------------------------------------------
class MergedSegments(object):
    """The result of mergeSegments.

    ``recode``: uint32, ``nb.maxSegId + 1`` rows, old id -> new id (0 for id 0 and, with ``segSize``, for ids without
    pixels); ``maxSegId``: M, the number of groups; ``representative``: uint32, ``M + 1`` rows, the smallest old id of
    every group; ``groupSize``: int64, the old ids in it (row 0 of both is 0); ``hist``: int64 pixel counts of the
    new ids as the segmentation's ``hist`` holds them, None when neither ``segSize`` nor ``segfile`` was given;
    ``neighbours``: the SegmentNeighbours of the groups, resident on the device; ``links``: the table's entries a < b
    that joined two segments; ``recordsSorted``: the entries a < b between different groups, handed to the sort;
    ``timings``: seconds per step; ``deviceMs``: GPU time of the kernels, ``stepDeviceMs`` the same per step (hook,
    renumber, contract, recode); ``segimg``: the recoded raster when ``segfile`` was an array and no ``outfile`` was
    given; ``outDev``: the recoded raster in device memory when the labels were there, in the form findSegmentNeighbours
    accepts (tiling.freeDeviceOutput releases it).

    For aggregateToGroups: ``membersOf(g)``, and ``memberOffsets`` (int64, ``maxSegId + 2``) with ``members`` (uint32):
    the old ids of every group in ascending order, as a CSR over the new ids.  Both arrays are None until the first
    call that needs them has brought them from the device.  ``aggregateTimings``: the last aggregateToGroups.  A
    result put together by hand needs ``recode`` and ``maxSegId``."""
    def __init__(self):
        self.recode = None
        self.maxSegId = 0
        self.representative = None
        self.groupSize = None
        self.hist = None
        self.neighbours = None
        self.links = 0
        self.recordsSorted = 0
        self.timings = {}
        self.deviceMs = 0.0
        self.stepDeviceMs = {}
        self.segimg = None
        self.outDev = None
        self.memberOffsets = None
        self.members = None
        self.aggregateTimings = {}
        self.groupsSerial = None
        self._groupsCtx = None

    def membersOf(self, group):
        """the old ids of one group, ascending: a view of ``members`` (fetched from the device by the first call)"""
        group = int(group)
        if group < 0 or group > self.maxSegId:
            raise PyShepSegNeighboursError("group {} is outside 0..{}".format(group, self.maxSegId))
        if self.memberOffsets is None:
            _fetchMembers(_lib.ctx(), _checkMerged(self), {})
        return self.members[int(self.memberOffsets[group]):int(self.memberOffsets[group + 1])]


class MergedSegmentsShare(MergedSegments):
    """A rank's result of distributed.mergeSegmentsDistributed / mergeSimilarSegmentsDistributed.  ``recode``,
    ``representative``, ``groupSize``, ``hist``, ``maxSegId``, ``links`` and ``recordsSorted`` are complete, the same on
    every rank and equal to the one-GPU function's on the whole table.  ``neighbours`` is a SegmentNeighboursShare: the
    rows of the contracted table of this rank's share of the new ids, resident on the rank's context as its share
    table.  ``outDev``: this rank's rows of the recoded raster in device memory, (pointer, rows, columns, bytes), None
    without rows; ``rowRange``: the image rows they are.  ``info``: this rank's figures of the exchange
    (distributed.deviceMerge)."""
    def __init__(self):
        MergedSegments.__init__(self)
        self.rowRange = None
        self.info = {}


def _integer(value, name):
    if isinstance(value, (bool, numpy.bool_)) or not isinstance(value, (int, numpy.integer)):
        raise PyShepSegNeighboursError("{} must be an integer (got {!r})".format(name, value))
    return int(value)


def _integerColumn(column, name, nrows):
    """a 1-D integer column of nrows values as contiguous int64"""
    column = numpy.asarray(column)
    if column.ndim != 1:
        raise PyShepSegNeighboursError("{} must be a 1-D array (got {} dimensions)".format(name, column.ndim))
    if column.dtype.kind not in 'iu':
        raise PyShepSegNeighboursError("{} has dtype {}: an integer type wanted".format(name, column.dtype))
    if len(column) != nrows:
        raise PyShepSegNeighboursError("{} has {} rows, the table maxSegId + 1 = {}".format(name, len(column), nrows))
    return numpy.ascontiguousarray(column.astype(numpy.int64, copy=False))


def _checkMergeArgs(nb, keyColumn, ignoreKey, minBorder, segSize, segfile, outfile, keyOptional=False):
    """(keys int64, ignore or None, minBorder, sizes int64 or None, the raster's labelsource.Labels or None):
    everything that can be refused before the GPU is touched.  keyOptional: ``keyColumn`` may be None (keys None)"""
    if not isinstance(nb, SegmentNeighbours):
        raise PyShepSegNeighboursError("nb must be a SegmentNeighbours")
    nrows = int(nb.maxSegId) + 1
    if len(nb.offsets) != nrows + 1 or len(nb.neighbours) != len(nb.borderLengths):
        raise PyShepSegNeighboursError("the table's arrays do not have the lengths of maxSegId {}".format(nb.maxSegId))
    return _checkMergeColumns(nrows, keyColumn, ignoreKey, minBorder, segSize, segfile, outfile, keyOptional)


def _checkMergeColumns(nrows, keyColumn, ignoreKey, minBorder, segSize, segfile, outfile, keyOptional=False):
    """_checkMergeArgs for a table of ``nrows`` ids, whatever holds its rows"""
    keys = None if (keyOptional and keyColumn is None) else _integerColumn(keyColumn, 'keyColumn', nrows)
    ignore = None
    if ignoreKey is not None:
        if keys is None:
            raise PyShepSegNeighboursError("ignoreKey needs a keyColumn")
        ignore = _integer(ignoreKey, 'ignoreKey')
        if ignore < -(1 << 63) or ignore >= (1 << 64):
            raise PyShepSegNeighboursError("ignoreKey {} is no 64-bit integer".format(ignore))
        if ignore >= (1 << 63):
            ignore -= 1 << 64           # (as a uint64 key column is read)
    minBorder = _integer(minBorder, 'minBorder')
    if minBorder < 1:
        raise PyShepSegNeighboursError("minBorder must be at least 1 (got {})".format(minBorder))
    minBorder = min(minBorder, (1 << 63) - 1)       # (no border length is larger)
    sizes = None
    if segSize is not None:
        sizes = _integerColumn(segSize, 'segSize', nrows)
        if len(sizes) and int(sizes.min()) < 0:
            raise PyShepSegNeighboursError("segSize holds a negative count")
    if outfile is not None and not (isinstance(outfile, str) and outfile.endswith('.npy')):
        raise PyShepSegNeighboursError("outfile must be None or a .npy path")
    raster = None
    if segfile is None:
        if outfile is not None:
            raise PyShepSegNeighboursError("outfile needs a segfile to recode")
    else:
        raster = _checkArgs(segfile, None)
        if isinstance(segfile, str) and outfile is None:
            raise PyShepSegNeighboursError("a .npy segfile is recoded into a file: outfile is required")
    return (keys, ignore, minBorder, sizes, raster)


def mergeSegments(nb, keyColumn, ignoreKey=None, minBorder=1, segSize=None, segfile=None, outfile=None,
                  chunkPixels=None):
    """
    Touching segments of one class become one object, on the GPU: a MergedSegments.

    ``nb`` is a SegmentNeighbours (uploaded when it is not the table on the device, as reduceOverNeighbours has it);
    ``keyColumn`` a 1-D integer array of ``maxSegId + 1`` values, the class of every segment, read as int64.  Entry
    (a, b, w) of the table is a link when ``key[a] == key[b]``, ``key[a] != ignoreKey`` and ``w >= minBorder``; a group
    is a connected component of the links over the ids 1..maxSegId, so a path of links joins two segments whose own
    border is below ``minBorder``.  ``segSize`` (``maxSegId + 1`` pixel counts, such as the segmentation's ``hist``):
    an id of size 0 belongs to no group and recodes to 0; without it every id is a vertex and one with an empty row
    is a group of one.  Groups are numbered 1..M in ascending order of their smallest member.  The table must name
    every pair from both sides, as every table of findSegmentNeighbours does.

    The contracted table (every entry between two groups adds its length to the groups' border) becomes the table
    resident on the device: ``result.neighbours`` goes into reduceOverNeighbours without an upload, ``nb`` is
    uploaded again when it is used.  When ``nb`` is the table of a raster, ``result.neighbours`` is array for array
    ``findSegmentNeighbours(recode[raster], nb.fourConnected, maxSegId=M)``.

    ``segfile`` (what findSegmentNeighbours takes) is recoded as well, in row blocks of ``chunkPixels`` pixels: an
    array comes back as ``result.segimg`` or goes to ``outfile`` (a ``.npy`` path); a ``.npy`` path needs ``outfile``;
    labels kept on the device are recoded into a second device raster, ``result.outDev``, unless ``outfile`` is
    given.  A label above ``nb.maxSegId`` raises PyShepSegNeighboursError with the largest such label.  Without
    ``segSize`` the new ``hist`` is counted in that pass.
    """
    (keys, ignore, minBorder, sizes, raster) = _checkMergeArgs(nb, keyColumn, ignoreKey, minBorder, segSize, segfile,
                                                                outfile)

    def links(c, S, M, counters, ms):
        c.check(c._L.shp_nbr_merge(c.handle, _lib.ptr(keys), S + 1, int(ignore is not None), 0 if ignore is None else ignore,
                                   minBorder, None if sizes is None else _lib.ptr(sizes), ctypes.byref(M),
                                   _lib.ptr(counters), _lib.ptr(ms)))
    return _mergeByLinks(nb, links, sizes, raster, outfile, chunkPixels)


def _mergeByLinks(nb, links, sizes, raster, outfile, chunkPixels):
    """What mergeSegments and mergeSimilarSegments share, which is everything but the link rule: ``links(c, S, M,
    counters, ms)`` makes the library's call that finds the groups of the resident table (M: c_uint32, counters: 2
    int64, ms: 3 float64 -- hook, renumbering, and what the rule spends before the hook)."""
    t0 = time.perf_counter()
    c = _lib.ctx()
    L = c._L
    res = MergedSegments()
    timings = {'upload': 0.0, 'uploaded': False, 'deviceMs': 0.0}
    _makeResident(c, nb, timings)
    S = int(nb.maxSegId)
    # the groups
    t1 = time.perf_counter()
    (M, counters, ms2) = (ctypes.c_uint32(0), numpy.zeros(2, dtype=numpy.int64), numpy.zeros(3, dtype=numpy.float64))
    links(c, S, M, counters, ms2)
    M = M.value
    (res.groupsSerial, res._groupsCtx) = (_groupSerials(c)[0], c.handle.value)
    timings['merge'] = time.perf_counter() - t1
    t1 = time.perf_counter()
    res.recode = numpy.empty(S + 1, dtype=numpy.uint32)
    res.representative = numpy.empty(M + 1, dtype=numpy.uint32)
    res.groupSize = numpy.empty(M + 1, dtype=numpy.int64)
    if sizes is not None:
        res.hist = numpy.empty(M + 1, dtype=numpy.int64)
    c.check(L.shp_nbr_merge_groups(c.handle, _lib.ptr(res.recode), _lib.ptr(res.representative), _lib.ptr(res.groupSize),
                                   None if res.hist is None else _lib.ptr(res.hist)))
    timings['groups'] = time.perf_counter() - t1
    # their table
    t1 = time.perf_counter()
    (nent, nrec, msc) = (ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_double(0))
    (nb.residentSerial, nb._residentCtx) = (None, None)
    c.check(L.shp_nbr_merge_contract(c.handle, ctypes.byref(nent), ctypes.byref(nrec), ctypes.byref(msc)))
    timings['contract'] = time.perf_counter() - t1
    t1 = time.perf_counter()
    offsets = numpy.empty(M + 2, dtype=numpy.int64)
    nbrs = numpy.empty(nent.value, dtype=numpy.uint32)
    lens = numpy.empty(nent.value, dtype=numpy.int64)
    c.check(L.shp_nbr_download(c.handle, _lib.ptr(offsets), _lib.ptr(nbrs), _lib.ptr(lens)))
    timings['download'] = time.perf_counter() - t1
    res.neighbours = SegmentNeighbours(offsets, nbrs, lens, M, nb.fourConnected, recordsSorted=nrec.value,
                                       deviceMs=msc.value)
    (res.neighbours.residentSerial, res.neighbours._residentCtx) = (_tableSerial(c), c.handle.value)
    res.maxSegId = M
    res.links = int(counters[0])
    res.recordsSorted = nrec.value
    res.stepDeviceMs = {'hook': float(ms2[0]), 'renumber': float(ms2[1]), 'contract': msc.value, 'recode': 0.0}
    if ms2[2]:
        res.stepDeviceMs['records'] = float(ms2[2])
    # the raster
    if raster is not None:
        t1 = time.perf_counter()
        _recodeRaster(c, res, raster, S, outfile, chunkPixels, countHist=sizes is None)
        timings['recode'] = time.perf_counter() - t1
    timings['total'] = time.perf_counter() - t0
    res.deviceMs = timings.pop('deviceMs') + sum(res.stepDeviceMs.values())
    res.timings = timings
    return res


def _recodeRaster(c, res, raster, S, outfile, chunkPixels, countHist):
    """the label raster through the groups' recode on the device, in the row blocks of labelsource.mapBlocks"""
    L = c._L
    nbytes = raster.nrows * raster.ncols * 4
    worst = [0]

    def recode(y0, y1, dseg, dout):
        """False once a label was above S: nothing is kept from then on, the blocks still run to find the largest"""
        (bad, ms) = (ctypes.c_uint32(0), ctypes.c_double(0))
        c.check(L.shp_nbr_merge_recode_dev(c.handle, dseg, (y1 - y0) * raster.ncols, dout, int(countHist), ctypes.byref(bad),
                                           ctypes.byref(ms)))
        res.stepDeviceMs['recode'] += ms.value
        worst[0] = max(worst[0], bad.value)
        return not worst[0]

    devOut = None
    with labelsource.LabelSource(c, raster) as src:
        try:
            if outfile is None and raster.devSeg is not None:
                devOut = tiling._devAlloc(c, nbytes)
            out = labelsource.mapBlocks(src, chunkPixels, recode, numpy.uint32, outfile=outfile, devOut=devOut)
            if worst[0]:
                raise PyShepSegNeighboursError("segment id {} is above maxSegId {}".format(worst[0], S))
            if countHist:
                res.hist = numpy.empty(res.maxSegId + 1, dtype=numpy.int64)
                c.check(L.shp_nbr_merge_groups(c.handle, None, None, None, _lib.ptr(res.hist)))
            (res.segimg, res.outDev) = (out, None if devOut is None else (devOut.value, raster.nrows, raster.ncols, nbytes))
            devOut = None
        finally:
            if devOut is not None:
                tiling._devRelease(c, devOut, nbytes)


# ---- touching segments that look alike merged into one (csrc/nbrmerge.h, MrgSimRule) --------------------------
MAX_DISTANCE_COLUMNS = 8


def _distanceColumns(distanceColumns, nrows):
    """the columns as contiguous float64 arrays of nrows values"""
    if isinstance(distanceColumns, numpy.ndarray) or not isinstance(distanceColumns, (list, tuple)):
        raise PyShepSegNeighboursError("distanceColumns must be a list of 1-D columns")
    if not 1 <= len(distanceColumns) <= MAX_DISTANCE_COLUMNS:
        raise PyShepSegNeighboursError("distanceColumns has {} columns: 1 to {} wanted".format(
            len(distanceColumns), MAX_DISTANCE_COLUMNS))
    out = []
    for (i, column) in enumerate(distanceColumns):
        if not isinstance(column, numpy.ndarray) or column.ndim != 1:
            raise PyShepSegNeighboursError("distance column {} must be a 1-D numpy array".format(i))
        if column.dtype not in (numpy.float64, numpy.float32) and column.dtype.kind not in 'iu':
            raise PyShepSegNeighboursError("distance column {} has dtype {}: float64, float32 or an integer type "
                                           "wanted".format(i, column.dtype))
        if len(column) != nrows:
            raise PyShepSegNeighboursError("distance column {} has {} rows, the table maxSegId + 1 = {}".format(
                i, len(column), nrows))
        out.append(numpy.ascontiguousarray(column, dtype=numpy.float64))
    return out


def _checkSimilarRule(distanceColumns, nrows, maxDistance, mutualNearest, ignoreValue):
    """(the columns as float64, ignoreValue or None, thr2 or None) of the similarity rule for a table of ``nrows`` ids"""
    columns = _distanceColumns(distanceColumns, nrows)
    if isinstance(mutualNearest, (bool, numpy.bool_)) is False:
        raise PyShepSegNeighboursError("mutualNearest must be True or False (got {!r})".format(mutualNearest))
    ignoreV = None if ignoreValue is None else _number(ignoreValue, 'ignoreValue')
    thr2 = None
    if maxDistance is None:
        if not mutualNearest:
            raise PyShepSegNeighboursError("maxDistance=None (no threshold) needs mutualNearest=True")
    else:
        md = numpy.float64(_number(maxDistance, 'maxDistance'))
        if not numpy.isfinite(md) or md < 0:
            raise PyShepSegNeighboursError("maxDistance must be finite and not negative (got {!r})".format(maxDistance))
        with numpy.errstate(over='ignore'):
            thr2 = float(md * md)
    return (columns, ignoreV, thr2)


def mergeSimilarSegments(nb, distanceColumns, maxDistance=None, mutualNearest=False, ignoreValue=None, keyColumn=None,
                         ignoreKey=None, minBorder=1, segSize=None, segfile=None, outfile=None, chunkPixels=None):
    """
    Touching segments that look alike become one object, on the GPU: a MergedSegments.  It is mergeSegments with
    another link rule; the groups' numbering, ``recode``, ``representative``, ``groupSize``, ``hist``, the contracted
    table that becomes the resident one and the recoded raster are mergeSegments', as are ``nb``, ``minBorder``,
    ``segSize``, ``segfile``, ``outfile`` and ``chunkPixels``.

    ``distanceColumns``: a list of 1 to 8 one-dimensional columns of ``maxSegId + 1`` values, float64, float32 or any
    integer type, each widened to float64.  A value is ignored when it is NaN or equals ``ignoreValue``; an id with an
    ignored value in any column links to nobody.  ``d2(a, b)`` starts at +0.0 and adds, for the columns in list order,
    ``t * t`` with ``t = x[a] - x[b]``, every operation rounded to float64 once; ``thr2 = float64(maxDistance) ** 2``.
    ``maxDistance`` must be finite and not negative; None (no threshold) is allowed with ``mutualNearest`` only.

    Entry (a, b, w) of the table is a candidate when ``w >= minBorder``, both ids have pixels (with ``segSize``),
    neither has an ignored value, ``d2`` is finite and, with ``keyColumn``, ``key[a] == key[b] != ignoreKey``.

    ``mutualNearest=False``: a candidate is a link when ``d2 <= thr2`` and the groups are the connected components
    of the links.  This is SINGLE LINKAGE: a chain of small steps joins segments that are further apart than
    ``maxDistance``, just as a path of links joins two segments whose own border is below ``minBorder``.

    ``mutualNearest=True``: ``best[a]`` is the candidate neighbour of a with the smallest ``d2``, the smallest id among
    equals; (a, b) is a link when ``best[a] == b``, ``best[b] == a`` and ``d2 <= thr2``.  A group then has one or two
    members: one round of pairwise merging.  The table must name every pair from both sides, as every table of
    findSegmentNeighbours does.

    Nothing depends on the order in which the GPU gets to the entries.  Columns for the groups:
    aggregateToGroups(result, ...); the next round: mergeSimilarSegments(result.neighbours, ..., segSize=result.hist).
    """
    (keys, ignoreK, minBorder, sizes, raster) = _checkMergeArgs(nb, keyColumn, ignoreKey, minBorder, segSize, segfile,
                                                                 outfile, keyOptional=True)
    (columns, ignoreV, thr2) = _checkSimilarRule(distanceColumns, int(nb.maxSegId) + 1, maxDistance, mutualNearest,
                                                 ignoreValue)
    cols = (ctypes.c_void_p * len(columns))(*[column.ctypes.data for column in columns])

    def links(c, S, M, counters, ms):
        c.check(c._L.shp_nbr_merge_similar(
            c.handle, cols, len(columns), S + 1, int(ignoreV is not None), 0.0 if ignoreV is None else ignoreV,
            int(thr2 is not None), 0.0 if thr2 is None else thr2, int(bool(mutualNearest)),
            None if keys is None else _lib.ptr(keys), int(ignoreK is not None), 0 if ignoreK is None else ignoreK, minBorder,
            None if sizes is None else _lib.ptr(sizes), ctypes.byref(M), _lib.ptr(counters), _lib.ptr(ms)))
    return _mergeByLinks(nb, links, sizes, raster, outfile, chunkPixels)


# ---- columns of the old ids carried to the groups (csrc/nbragg.h) ---------------------------------------------
# statName -> (bit of the C call's mask, dtype of the column; None: int64 for an integer column, float64 otherwise)
AGGREGATE_STATS = {'count': (0, numpy.int64), 'weight': (1, numpy.int64), 'min': (2, numpy.float64),
                   'max': (3, numpy.float64), 'sum': (4, None), 'mean': (5, numpy.float64),
                   'weightedmean': (6, numpy.float64)}


def _aggregateType(dtype):
    """the library's type code of a column (integers of any width go as int64), None for a dtype it does not take"""
    if dtype in _COLUMN_TYPES:
        return _COLUMN_TYPES[dtype]
    return _COLUMN_TYPES[numpy.dtype(numpy.int64)] if dtype.kind in 'iu' else None


def _groupSerials(c):
    """(serial of the groups the context holds, serial of the groups whose member list it holds), None for none"""
    (groups, members) = (ctypes.c_uint64(0), ctypes.c_uint64(0))
    c.check(c._L.shp_nbr_groups_serial(c.handle, ctypes.byref(groups), ctypes.byref(members)))
    return (groups.value or None, members.value or None)


def _checkMerged(merged):
    if not isinstance(merged, MergedSegments) or not isinstance(merged.recode, numpy.ndarray):
        raise PyShepSegNeighboursError("merged must be a MergedSegments")
    M = _integer(merged.maxSegId, 'merged.maxSegId')
    if merged.recode.ndim != 1 or merged.recode.dtype != numpy.uint32 or not 0 <= M < max(len(merged.recode), 1):
        raise PyShepSegNeighboursError("merged.recode must be a 1-D uint32 array with more rows than merged.maxSegId")
    return merged


def _residentMembers(c, merged, timings):
    """the member list of ``merged`` on the device: there already, built from the groups the last merge call left
    there, or -- for an older result -- from ``merged.recode``, uploaded"""
    (groups, members) = _groupSerials(c)
    mine = merged.groupsSerial if merged._groupsCtx == c.handle.value else None
    timings.update(uploaded=False, built=False, buildDeviceMs=0.0)
    if mine is not None and mine == members:
        return
    (serial, n, ms) = (ctypes.c_uint64(0), ctypes.c_int64(0), ctypes.c_double(0))
    if mine is not None and mine == groups:
        c.check(c._L.shp_nbr_members_build(c.handle, None, 0, 0, ctypes.byref(serial), ctypes.byref(n), ctypes.byref(ms)))
    else:
        recode = numpy.ascontiguousarray(merged.recode)
        rc = c._L.shp_nbr_members_build(c.handle, _lib.ptr(recode), len(recode), int(merged.maxSegId), ctypes.byref(serial),
                                        ctypes.byref(n), ctypes.byref(ms))
        if rc != 0:
            raise PyShepSegNeighboursError((c._L.shp_last_error(c.handle) or b'').decode())
        timings['uploaded'] = True
        (merged.groupsSerial, merged._groupsCtx) = (serial.value, c.handle.value)
    timings.update(built=True, buildDeviceMs=ms.value)


def _fetchMembers(c, merged, timings):
    _residentMembers(c, merged, timings)
    offsets = numpy.empty(int(merged.maxSegId) + 2, dtype=numpy.int64)
    members = numpy.empty(numpy.count_nonzero(merged.recode), dtype=numpy.uint32)
    c.check(c._L.shp_nbr_members_download(c.handle, _lib.ptr(offsets), _lib.ptr(members) if len(members) else None))
    (merged.memberOffsets, merged.members) = (offsets, members)


def aggregateToGroups(merged, columnSelections, weights=None, ignoreValue=None, missingStatsValue=-9999):
    """
    Columns of the old segments carried to the groups of a merge, on the GPU: a dictionary outName -> numpy array of
    ``merged.maxSegId + 1`` rows.

    ``merged`` is the MergedSegments of mergeSegments or mergeSimilarSegments.  ``columnSelections`` has the form
    reduceOverNeighbours takes, ``[(column, [(outName, statName), ...]), ...]``; a column holds a value for every OLD
    id (``len(merged.recode)`` values: float64, float32 or an integer type, integers read as int64).  ``weights``: an
    integer column of the same length with values of 0 or more, typically the ``segSize`` the merge was given; None:
    every weight is 1.

    The members of group g are the old ids i with ``recode[i] == g`` in ascending order (``merged.membersOf(g)``); ids
    that recode to 0 are in no group.  Over the members whose value is not ignored (NaN, or equal to ``ignoreValue``):
    ``count`` of them and ``weight`` = sum w (int64); ``min``, ``max`` (float64); ``sum``: exact int64, wrapping as
    numpy's, for an integer column and float64 otherwise; ``mean`` = (float64 sum) / count; ``weightedmean`` =
    sum(float64(w) v) / sum w, each product rounded before it is added.  Row 0, and a group without a value (for
    ``weightedmean`` also one whose weights sum to 0), hold ``missingStatsValue`` in the float statistics and 0 in the
    integer ones.  The weighted mean of a ``Band_n_mean`` column by ``segSize`` is the merged object's band mean; the
    class of a group after a key merge is ``keys[merged.representative]``.

    The float sums are float64 in the order csrc/nbrreduce.h states for a row, here the group's member list: a group's
    result depends on nothing but the group.  The member list is built on the device once per merge result and stays
    there until the next merge call; on an older result ``recode`` is uploaded and the list rebuilt, with the same
    bits as the result.  The resident neighbour table is not touched.
    """
    return _aggregateOnContext(None, merged, columnSelections, weights, ignoreValue, missingStatsValue)


def _aggregateOnContext(ctx, merged, columnSelections, weights, ignoreValue, missingStatsValue):
    """aggregateToGroups on the context ``ctx`` (None: the calling thread's)"""
    merged = _checkMerged(merged)
    nrows = len(merged.recode)
    (plan, ignore, missing) = _planSelections(nrows, columnSelections, ignoreValue, missingStatsValue, AGGREGATE_STATS,
                                              _aggregateType)
    w = None
    if weights is not None:
        w = _integerColumn(weights, 'weights', nrows)
        if len(w) and int(w.min()) < 0:
            raise PyShepSegNeighboursError("weights holds a negative value")
    t0 = time.perf_counter()
    c = _lib.ctx() if ctx is None else ctx
    L = c._L
    timings = {'deviceMs': 0.0}
    _residentMembers(c, merged, timings)
    t1 = time.perf_counter()
    out = {}
    ngroups = int(merged.maxSegId) + 1
    for (column, ctype, picked) in plan:
        if ctype == _COLUMN_TYPES[numpy.dtype(numpy.int64)]:
            column = numpy.ascontiguousarray(column.astype(numpy.int64, copy=False))
        arrays = {}
        mask = 0
        ptrs = (ctypes.c_void_p * len(AGGREGATE_STATS))()
        for (_outName, bit, dtype) in picked:
            if bit not in arrays:
                if dtype is None:
                    dtype = numpy.int64 if column.dtype.kind in 'iu' else numpy.float64
                arrays[bit] = numpy.empty(ngroups, dtype=dtype)
                ptrs[bit] = arrays[bit].ctypes.data
                mask |= 1 << bit
        ms = ctypes.c_double(0)
        c.check(L.shp_nbr_aggregate(c.handle, _lib.ptr(column), ctype, nrows, None if w is None else _lib.ptr(w),
                                    int(ignore is not None), 0.0 if ignore is None else ignore, missing, mask, ptrs,
                                    ctypes.byref(ms)))
        timings['deviceMs'] += ms.value
        first = set()
        for (outName, bit, _dtype) in picked:
            out[outName] = arrays[bit] if bit not in first else arrays[bit].copy()
            first.add(bit)
    timings['aggregate'] = time.perf_counter() - t1
    timings['total'] = time.perf_counter() - t0
    merged.aggregateTimings = timings
    return out
