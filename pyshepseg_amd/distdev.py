"""What the multi-rank job modules (dist_stats, dist_spatial, dist_subset, dist_neighbours, dist_colour) and the
driver (distributed) share: the pure planning functions (id shares, halo rows, row checks, the output stage's
pieces and overview rectangles) and the steps every "device path for ONE rank" is made of -- device scratch, the
padded all-gather of records, the resident histogram, the column block, errors raised on every rank.  No helper
here makes a collective the caller does not see in its own text, bar gatherRecords' one allgather_dev and the
functions named ...OnAllRanks."""
import ctypes
import os

import numpy

from . import _lib
from . import tiling


_DTYPE_SIZE = {0: 1, 1: 2, 2: 2, 3: 4, 4: 4}


def _addr(p):
    """a device address as an int (None, an int or a ctypes.c_void_p)"""
    if p is None:
        return 0
    return int(p.value or 0) if hasattr(p, 'value') else int(p)


# ------------------------------------------------------------------------------------------
# planning: id shares, halo rows, the ranks' rows
# ------------------------------------------------------------------------------------------
def idRange(rank, world, maxSegId):
    """This rank's share [lo, hi) of the id space 0..maxSegId for the reduction of straddling segments
    ('GPU g owns ids in [g S / N, (g + 1) S / N)')."""
    ns = int(maxSegId) + 1
    return (rank * ns) // world, ((rank + 1) * ns) // world


def spatialHaloPlan(rowRanges, rank, nRows, above, below):
    """Where rank ``rank`` finds the halo rows of the spatial statistics.  rowRanges: every rank's output rows
    (outLo, outHi); ``above`` / ``below``: rows needed above / below the shard (mean coordinates 0 / 0, edge
    pixels 1 / 1, the variogram 0 / maxDist).  Every rank contributes its first min(h, below) rows to slot rows
    [0, below) and its last min(h, above) rows to slot rows [below, below + above) of one all-gather of
    ``slot`` = above + below rows per rank; a halo may span several ranks (thin or empty shards) and stops at
    the image's border.  Returns a dict: 'above' / 'below' = halo rows this rank gets (ha, hb), 'slot',
    'send' = [(own row, slot row, rows)], 'recvAbove' / 'recvBelow' = [(halo row, source rank, slot row,
    rows)] (halo row 0 = global row outLo - ha, resp. outHi).  Output rows shared by several ranks (tile
    sharding) are refused when a halo is needed, as are rows of a halo that no rank holds."""
    from .tilingstats import PyShepSegStatsError
    ranges = [(int(a), int(b)) for (a, b) in rowRanges]
    (above, below, nRows) = (int(above), int(below), int(nRows))
    (lo, hi) = ranges[rank]
    live = sorted((a, b) for (a, b) in ranges if b > a)
    if above or below:
        for (x, y) in zip(live, live[1:]):
            if x[1] > y[0]:
                raise PyShepSegStatsError(
                    "edge pixels and the variogram need ranks with disjoint output rows (rows %d..%d and %d..%d "
                    "overlap): run the segmentation with SHEPSEG_SHARD=rows" % (x[0], x[1], y[0], y[1]))
    h = max(hi - lo, 0)
    plan = {'slot': above + below, 'send': [], 'recvAbove': [], 'recvBelow': [], 'above': 0, 'below': 0}
    first, last = min(h, below), min(h, above)
    if first:
        plan['send'].append((0, 0, first))
    if last:
        plan['send'].append((h - last, below, last))
    if h == 0:
        return plan

    def owner(y):
        for (r, (a, b)) in enumerate(ranges):
            if a <= y < b:
                return r
        raise PyShepSegStatsError("row %d of the spatial statistics' halo is held by no rank" % y)

    def runs(rows, slotRowOf):
        out = []
        for (k, y) in enumerate(rows):
            o = owner(y)
            sr = slotRowOf(o, y)
            if out and out[-1][1] == o and out[-1][2] + out[-1][3] == sr:
                out[-1][3] += 1
            else:
                out.append([k, o, sr, 1])
        return [tuple(x) for x in out]
    up = list(range(max(0, lo - above), lo))
    dn = list(range(hi, min(nRows, hi + below)))
    plan['above'], plan['below'] = len(up), len(dn)
    plan['recvAbove'] = runs(up, lambda o, y: below + y - (ranges[o][1] - min(ranges[o][1] - ranges[o][0], above)))
    plan['recvBelow'] = runs(dn, lambda o, y: y - ranges[o][0])
    return plan


def disjointRowsError(rowRanges, what):
    """None when the ranks' output rows (outLo, outHi) do not overlap, else the message that refuses them for
    ``what`` (tile-sharded runs share rows)."""
    live = sorted((int(a), int(b)) for (a, b) in rowRanges if b > a)
    for (x, y) in zip(live, live[1:]):
        if x[1] > y[0]:
            return ("%s needs ranks with disjoint output rows (rows %d..%d and %d..%d overlap): run the "
                    "segmentation with SHEPSEG_SHARD=rows" % (what, x[0], x[1], y[0], y[1]))
    return None


def _rowsCoverError(ranges, nRows):
    """None when the ranks' output rows tile 0..nRows without a gap (they are known not to overlap)"""
    at = 0
    for (a, b) in sorted((a, b) for (a, b) in ranges if b > a):
        if a != at:
            return "rows %d..%d of the raster are held by no rank" % (at, a)
        at = b
    if at != nRows:
        return "rows %d..%d of the raster are held by no rank" % (at, nRows)
    return None


def allRows(ranges, nRows):
    """the raster's rows: ``nRows``, or the largest outHi of the ranks' (outLo, outHi) when that is None"""
    return int(max(b for (a, b) in ranges) if nRows is None else nRows)


# ------------------------------------------------------------------------------------------
# errors raised on every rank
# ------------------------------------------------------------------------------------------
def raiseFirst(Err, errs):
    """Raise the first non-empty message of ``errs`` (every rank's, already gathered) as Err; no collective."""
    for e in errs:
        if e:
            raise Err(e)


def histogramMismatch(over, px, hpx):
    """None, or the message for a histogram that cannot belong to the labels: ``over`` ids with more pixels on one
    rank than it gives them, ``px`` labelled pixels of all ranks against its ``hpx``."""
    if over or px != hpx:
        return ("the segment histogram does not match the label raster (%d ids with more pixels on one rank "
                "than the histogram says; %d labelled pixels, %d in the histogram)" % (over, px, hpx))
    return None


_SAME_TYPE_ERRORS = (TypeError, ValueError, IndexError, OSError, tiling.PyShepSegTilingError,
                     _lib.ShepsegHipError)      # (and tilingstats.PyShepSegStatsError: _raiseFirstError adds it)


def _raiseOnAllRanks(comm, err):
    """All-gather this rank's exception (or None); the first rank's is raised on every rank, with its type when
    that is one of _SAME_TYPE_ERRORS (else as tiling.PyShepSegTilingError)."""
    _raiseFirstError(comm, err, comm.allgather_obj(None if err is None else (type(err).__name__, str(err))))


def _raiseFirstError(comm, err, got):
    """The raising half of _raiseOnAllRanks for a caller whose own collective carried the errors: ``got`` = every
    rank's (type name, message) or None."""
    bad = [(r, x) for (r, x) in enumerate(got) if x is not None]
    if not bad:
        return
    (r, (name, msg)) = bad[0]
    if err is not None and r == comm.rank:
        raise err
    from . import tilingstats
    types = {t.__name__: t for t in _SAME_TYPE_ERRORS + (tilingstats.PyShepSegStatsError,)}
    typ = types.get(name, tiling.PyShepSegTilingError)
    raise typ(msg if name in types else '%s: %s' % (name, msg))


def _stepOnAllRanks(comm, outname, fn, Err):
    """fn() on this rank, then an all-gather of what failed (a collective: every rank calls it): the first
    rank's error is raised as Err on every rank, so none is left waiting in a later collective"""
    err = None
    try:
        fn()
    except Exception as e:      # noqa: B902  (raised below, on every rank)
        err = '%s: %s' % (type(e).__name__, e)
    errs = [(r, x) for (r, x) in enumerate(comm.allgather_obj(err)) if x]
    if errs:
        raise Err("writing %s failed on rank %d: %s" % (outname, errs[0][0], errs[0][1]))


def _writeRows(comm, outname, rows, a, shape):
    """rank 0 creates the .npy file, then every rank writes its rows; a collective before and after (built from
    allgather_obj), errors raised on every rank"""
    from . import subset

    def step(fn):
        _stepOnAllRanks(comm, outname, fn, subset.PyShepSegSubsetError)

    def create():
        if comm.rank == 0:
            f = numpy.lib.format.open_memmap(outname, mode='w+', dtype=numpy.uint32, shape=shape)
            f.flush()
            del f

    def write():
        if len(rows):
            f = numpy.lib.format.open_memmap(outname, mode='r+')
            f[a:a + len(rows)] = rows
            f.flush()
            del f
    step(create)
    step(write)


# ------------------------------------------------------------------------------------------
# the steps of a device path for ONE rank
# ------------------------------------------------------------------------------------------
def deviceComm(comm, c):
    """``comm`` when it moves device buffers itself, else staged through the host of context ``c``"""
    from . import comm as _comm
    return comm if getattr(comm, 'onDevice', False) else _comm.HostStagedDev(comm, c)


class Scratch(object):
    """Device scratch of one call on context ``c``, from and back to the driver's cache of device blocks (a
    1.2-GB hipMalloc per call otherwise): ``with Scratch(c) as s`` releases every block of s.alloc on exit, normal
    or raising, bar those handed to s.keep."""

    def __init__(self, c):
        (self.c, self.blocks) = (c, [])

    def __enter__(self):
        return self

    def alloc(self, nbytes):
        p = tiling._devAlloc(self.c, nbytes)
        self.blocks.append((p, nbytes))
        return p

    def keep(self, p):
        """block ``p`` survives the exit: whoever gets it releases it"""
        self.blocks = [(q, n) for (q, n) in self.blocks if q is not p]
        return p

    def __exit__(self, *exc):
        (blocks, self.blocks) = (self.blocks, [])
        for (p, nbytes) in blocks:
            tiling._devRelease(self.c, p, nbytes)
        return False


def gatherRecords(s, c, comm, src, count, counts, itemBytes, inPlaceAlone=False):
    """This rank's ``count`` records of itemBytes at device address ``src``, padded to the largest of the ranks'
    ``counts`` and all-gathered (a rank without records still takes part): (d_all or None, slot), None when no
    rank has any -- then nothing is allocated, copied or gathered.  inPlaceAlone: a world of one gets its own
    block where it lies, (src, count)."""
    slot = max(counts)
    if slot == 0:
        return None, 0
    if inPlaceAlone and comm.world == 1:
        return src, count
    d_send = s.alloc(slot * itemBytes)
    d_all = s.alloc(comm.world * slot * itemBytes)
    if count:
        c.check(c._L.shp_dev_copy(c.handle, d_send, src, count * itemBytes))
    comm.allgather_dev(d_send.value, d_all.value, slot * itemBytes)
    return d_all, slot


def residentHist(s, c, hist, host=False):
    """The global histogram in device memory: ``hist`` is a host array, uploaded into scratch, or ('dev', address,
    length), taken as it is and never released.  Returns (d_hist, ns, h32); h32 is the uint32 host copy, which
    a device histogram gets only with ``host`` (None otherwise)."""
    if isinstance(hist, tuple):
        (d_hist, ns, h32) = (ctypes.c_void_p(hist[1]), int(hist[2]), None)
        if host:
            h32 = numpy.empty(ns, dtype=numpy.uint32)
            c.check(c._L.shp_dev_download(c.handle, _lib.ptr(h32), d_hist, ns * 4))
        return d_hist, ns, h32
    h32 = numpy.ascontiguousarray(hist, dtype=numpy.uint32)
    ns = len(h32)
    d_hist = s.alloc(ns * 4)
    c.check(c._L.shp_dev_upload(c.handle, d_hist, _lib.ptr(h32), ns * 4))
    return d_hist, ns, h32


def colWords(nInt, nFloat, ns):
    """int64 words of the column block: nInt int64 rows, then nFloat float32 rows, of ns values"""
    return ((nInt * 8 + nFloat * 4) * ns + 7) // 8


def allocColumns(s, c, words):
    """the column block in scratch, its last word zero (the float rows may end half-way into it)"""
    d_cols = s.alloc(words * 8)
    c.check(c._L.shp_dev_memset(c.handle, ctypes.c_void_p(d_cols.value + (words - 1) * 8), 0, 8))
    return d_cols


def fetchColumns(c, d_cols, nInt, nFloat, ns, fetch):
    """the column block on the host: (ic int64 (nInt, ns), fc float32 (nFloat, ns)); (None, None) without fetch"""
    if not fetch:
        return None, None
    ic = numpy.empty((nInt, ns), dtype=numpy.int64)
    fc = numpy.empty((nFloat, ns), dtype=numpy.float32)
    if nInt:
        c.check(c._L.shp_dev_download(c.handle, _lib.ptr(ic), d_cols, ic.nbytes))
    if nFloat:
        c.check(c._L.shp_dev_download(c.handle, _lib.ptr(fc), ctypes.c_void_p(d_cols.value + nInt * 8 * ns), fc.nbytes))
    return ic, fc


# ------------------------------------------------------------------------------------------
# planning of the output stage: this rank's pieces of the mosaic, the overview rectangles its tiles own
# ------------------------------------------------------------------------------------------
def _overviewBlock(tileInfo, overlapSize, lvl, col, row, ovw, ovh):
    """(x0, y0, x1, y1, sx, sy): the block k_overview_window writes for a tile at one level -- layer pixels
    [x0, x1) x [y0, y1), pixel (x0 + c, y0 + r) sampling raster pixel (sx + c lvl, sy + r lvl) -- or None when
    the tile's trimmed window is no larger than lvl / 2 in one direction (the kernel writes nothing)."""
    (xpos, ypos, xs, ys) = tileInfo.getTile(col, row)
    (top, bottom, left, right, xout, yout) = tiling.trimmedWindow(tileInfo, col, row, xpos, ypos, xs, ys, overlapSize)
    (w, h, o) = (right - left, bottom - top, lvl // 2)
    nsr = (h - o + lvl - 1) // lvl if h > o else 0
    nsc = (w - o + lvl - 1) // lvl if w > o else 0
    (x0, y0) = (xout // lvl, yout // lvl)
    (x1, y1) = (min(x0 + nsc, ovw), min(y0 + nsr, ovh))
    if x1 <= x0 or y1 <= y0:
        return None
    return (x0, y0, x1, y1, xout + o, yout + o)


def overviewPlan(tileInfo, overlapSize, lvl, tiles):
    """The part of each tile's overview block that the tile owns at level ``lvl``: one entry per (col, row) of
    ``tiles``, (x0, y0, x1, y1, sx, sy) -- layer pixels [x0, x1) x [y0, y1), pixel (x0 + c, y0 + r) sampling
    raster pixel (sx + c lvl, sy + r lvl) -- or None when it owns nothing.

    The one-GPU driver writes the blocks tile by tile in row-major (chain) order, a later block over an earlier
    one; a tile owns a pixel when it is the last tile whose block covers it, so ranks that write their tiles'
    owned parts at the same time make the same layer.  Tiles of one tile column share xout and the window
    width, tiles of one tile row share yout and the window height, so what a tile owns is its block clipped at
    the first column of the next non-empty block to its right (same tile row) and at the first row of the next
    non-empty block below it (same tile column); a block is empty when its window is no larger than lvl / 2."""
    (ncols, nrows) = (tileInfo.ncols, tileInfo.nrows)
    nCols = max(x + xs for (x, _y, xs, _ys) in tileInfo.tiles.values())
    nRows = max(y + ys for (_x, y, _xs, ys) in tileInfo.tiles.values())
    (ovw, ovh) = ((nCols + lvl - 1) // lvl, (nRows + lvl - 1) // lvl)
    memo = {}

    def block(c, r):
        if (c, r) not in memo:
            memo[(c, r)] = _overviewBlock(tileInfo, overlapSize, lvl, c, r, ovw, ovh)
        return memo[(c, r)]
    out = []
    for (col, row) in tiles:
        b = block(col, row)
        if b is None:
            out.append(None)
            continue
        (x0, y0, x1, y1, sx, sy) = b
        for c in range(col + 1, ncols):
            nb = block(c, row)
            if nb is not None:
                x1 = min(x1, nb[0])
                break
        for r in range(row + 1, nrows):
            nb = block(col, r)
            if nb is not None:
                y1 = min(y1, nb[1])
                break
        out.append((x0, y0, x1, y1, sx, sy) if x1 > x0 and y1 > y0 else None)
    return out


def checkNpyOutfile(outfile):
    """The output the multi-rank driver writes: a .npy path whose directory exists and is writable (every rank
    must see it).  Raises tiling.PyShepSegTilingError; creates nothing."""
    Err = tiling.PyShepSegTilingError
    if not isinstance(outfile, str) or not outfile.endswith('.npy'):
        raise Err("the multi-rank driver writes a .npy file that every rank can write (got %r); GDAL formats "
                  "and outfile=None are not supported" % (outfile,))
    d = os.path.dirname(os.path.abspath(outfile))
    if not os.path.isdir(d) or not os.access(d, os.W_OK):
        raise Err("cannot write %r: %s is not a writable directory" % (outfile, d))


def _mosaicPieces(dres):
    """What this rank writes of the mosaic: [(y0, y1, x0, x1)] -- its output rows in one piece when it holds
    whole tile rows (no other rank writes them), else its tiles' trimmed windows (ranks share output rows)"""
    (t0, t1) = dres.tileRange
    (lo, hi) = dres.outRows
    ti = dres.tileInfo
    if t1 <= t0 or hi <= lo:
        return []
    if t0 % ti.ncols == 0 and t1 % ti.ncols == 0:
        return [(lo, hi, 0, dres.nCols)]
    out = []
    for t in range(t0, t1):
        (col, row) = (t % ti.ncols, t // ti.ncols)
        (top, bottom, left, right, xout, yout) = tiling.trimmedWindow(ti, col, row, *ti.getTile(col, row),
                                                                      dres.overlapSize)
        if bottom > top and right > left:
            out.append((yout, yout + bottom - top, xout, xout + right - left))
    return out


def overviewTable(dres, levels):
    """This rank's overview rectangles of every level, for engine.overviewRects: (table int64 (n, 6) rows
    {src0, rowStep, colStep, nrows, ncols, dst0} relative to the output rows the engine holds (image row
    outRows[0] first), [(level, x0, y0, x1, y1)] in the same order, packed pixel count)"""
    (t0, t1) = dres.tileRange
    ti = dres.tileInfo
    tiles = [(t % ti.ncols, t // ti.ncols) for t in range(t0, t1)]
    (lo, nCols) = (dres.outRows[0], dres.nCols)
    (rows, where, at) = ([], [], 0)
    for lvl in levels:
        for p in overviewPlan(ti, dres.overlapSize, lvl, tiles):
            if p is None:
                continue
            (x0, y0, x1, y1, sx, sy) = p
            rows.append(((sy - lo) * nCols + sx, lvl * nCols, lvl, y1 - y0, x1 - x0, at))
            where.append((lvl, x0, y0, x1, y1))
            at += (y1 - y0) * (x1 - x0)
    return numpy.array(rows, dtype=numpy.int64).reshape(-1, 6), where, at


def overviewHoles(tileInfo, overlapSize, lvl):
    """The pixels of the overview layer of level ``lvl`` that no tile's block covers (they keep the file's fill
    value, the null label): (columns, rows) as sorted int arrays -- a pixel is uncovered when its column or its row
    is listed.  The blocks of one tile column share their columns and the blocks of one tile row their rows
    (overviewPlan), so the covered pixels are the product of the covered columns and the covered rows."""
    nCols = max(x + xs for (x, _y, xs, _ys) in tileInfo.tiles.values())
    nRows = max(y + ys for (_x, y, _xs, ys) in tileInfo.tiles.values())
    (ovw, ovh) = ((nCols + lvl - 1) // lvl, (nRows + lvl - 1) // lvl)
    colCovered = numpy.zeros(ovw, dtype=bool)
    rowCovered = numpy.zeros(ovh, dtype=bool)
    for row in range(tileInfo.nrows):
        for col in range(tileInfo.ncols):
            b = _overviewBlock(tileInfo, overlapSize, lvl, col, row, ovw, ovh)
            if b is not None:
                colCovered[b[0]:b[2]] = True
                rowCovered[b[1]:b[3]] = True
    return numpy.flatnonzero(~colCovered), numpy.flatnonzero(~rowCovered)
