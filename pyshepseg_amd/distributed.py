"""Multi-GPU tiled Shepherd segmentation: one process per GPU, RCCL over xGMI bound directly
behind the C-ABI (pyshepseg_amd/comm.py: RcclComm; SocketComm in the CPU tests).

What shards and what does not
-----------------------------
* Tiles are independent once the global k-means model is known (reference tiling.py:1430-1453),
  so the tiles, in row-major order, are dealt to ranks in contiguous ranges balanced by area
  (whole tile rows when there are too few tiles per rank); every rank holds only the rows of the
  raster its tiles need and the rows of the stitched output they write.  No collective on that
  path.
* The cross-tile stitch is specified sequentially (reference stitchTiles, tiling.py:979-1043:
  every tile's new ids start after the largest id of all earlier tiles, and shared segments
  take the id the tile above / to the left already gave them).  Two forms, same result:
  - sequential: rank r stitches its tiles once it has received, from the rank holding the tiles
    before, the running maxSegId, the recoded bottom overlap strips of that rank's last ncols
    tiles (the top neighbours of this rank's first tiles) and, when this rank starts in the middle
    of a tile row, the right strip of the tile before -- point-to-point send/recv, <= 25 MB per
    strip -- and passes its own on at the end;
  - parallel (default with more than one rank): tile t numbers its new segments from a
    PROVISIONAL base t * stride (stride = 2^32 / number of tiles), so its chain step needs the
    strips of the tiles above and to the left only -- a rank starts as soon as the first strip of
    the previous rank's last row arrives, strips travel tile by tile, and a rank takes its tiles
    along anti-diagonals so that the tiles of its last row are ready two steps apart instead of a
    row apart (SHEPSEG_CHAIN_ORDER=rowmajor: the old order).  Every tile reports K_t =
    ids handed out and R_t = the largest of them present in its trimmed window; an all-gather
    later, if K_t == R_t everywhere, the sequential run would have found maxSegId = sum of the
    earlier K (the reference advances it to trimmed.max()), the provisional ids are in the same
    order as the final ones (ties in the mode are broken by id) and no two of them collide, so
    id -> base[id / stride] + id % stride over the output gives the identical raster.  A tile
    with K_t != R_t (the reference then reuses ids: tests/golden/stitch_quirk_empties) or with
    more local segments than the stride sends every rank back to the sequential form.
  A final all-reduce sums the per-rank histograms.
* The k-means fit: every rank gets the whole sub-sample (all-gathered from the ranks' slices).  On device
  transports (RCCL) the fit's E-step is sharded by sample rows over the ranks, its labels all-gathered on the
  device every iteration, and every rank runs the same M-step: the same model everywhere, no broadcast
  (shp_kmeans_fit_planar_dist).  Other transports fit on rank 0 and broadcast the centres.

The driver below is engine-agnostic: ``HipEngine`` drives libshepseg_hip.so on this rank's GPU;
the CPU tests plug in an engine built on the oracle (tests/dist_oracle_engine.py) to exercise the
sharding / exchange logic with several ranks over sockets.

The engine
----------
What the two drivers below call on it (j: a tiling.makeTileJobs job; strip: the engine's handle of a
recoded overlap strip, None for no neighbour; win: tiling.trimmedWindow's six numbers):
  setup(tileInfo, jobs, total, yLo, yHi, outLo, outHi, nCols, overlapSize): first call of a run;
      raster rows [yLo, yHi), output rows [outLo, outHi) reading 0 where no tile of this rank writes.
  subsample(rows, cols) -> (nBands, len(rows), len(cols)); fit(img, numClusters, imgNullVal,
      fixedKMeansInit) -> a model with cluster_centers_ (optional fitSharded: the E-step over the ranks).
  startSegmentation(centres, msd, imgNullVal, fourConnected, minSegmentSize) may return at once;
      waitTile(j) returns when tile j is segmented and raises if it failed.
  setMaxSegId(v); stitchTile(j, top, left, win, simple): tile j's new ids follow the running maxSegId,
      its trimmed window goes to the output, the running maxSegId becomes that window's largest id;
      getMaxSegId() waits for the chain.  bottomStripOf(j) / rightStripOf(j): strips of local tiles.
  beginProvisional(stride, ntAll); stitchTileAt(j, top, left, win, t, stride, slot): stitchTile
      numbering after t * stride, its counts (K ids handed out, R the largest in the window, both
      minus the base) in slot `slot`; tileCounts(n) -> the n (K, R) pairs.
  sendStrip(comm, dst, item, j) / recvStrip(comm, src, item) -> strip: one boundaryPlan item.  An
      engine whose transfers may return before the data has moved also provides drainStrips(),
      which returns once all of it has; without one they count as done on return.
  renumber(stride, base): id -> base[id / stride] + id % stride over the output rows;
      renumberKept(stride, base, keptJobs, recvStrips): the same over the output rows, the strips of
      exactly keptJobs and exactly recvStrips, and no other buffer (final ids must stay as they are).
  sendBoundary(comm, dst, maxSegId, items) / recvBoundary(comm, src, plan) -> (maxSegId,
      {(kind, col, row): strip}): maxSegId, then the strips in plan order.
  histogram(maxSegId) -> pixel counts per id of the output rows (after finish too, if kept);
      finish(): the run's buffers released, bar a kept output.
  outputRows(y0, y1) -> image rows [y0, y1) of the kept output (inside outRows), uint32, on the host;
      overviewRects(table, npacked) -> the pixels of a table of overview rectangles (overviewTable), packed:
      writeOutputDistributed, after finish.

The jobs on the kept output
---------------------------
Each has a module of its own, built on the steps of distdev.py, and asks the engine for one more method:
  dist_stats: calcPerSegmentStatsDistributed[Bands] -- localStatsBands, gatherFlaggedBands, statsOfPairsBands
      (optional statsBandsOnDevice), or localStats, gatherFlagged, statsOfPairs (the protocol: _distributedStats).
  dist_spatial: calcPerSegmentSpatialStatsDistributed -- spatialOnDevice.
  dist_subset: subsetImageDistributed -- subsetOnDevice.
  dist_neighbours: findSegmentNeighboursDistributed -- neighboursOnDevice; merge...Distributed -- mergeOnDevice;
      reduceOverNeighboursDistributed and aggregateToGroupsDistributed need only the engine's context ``c``.
  dist_colour: writeColorTableFromRatColumnsDistributed, renderColourTableDistributed -- colourTableOnDevice,
      renderOnDevice.
  dist_shapes: calcSegmentShapesDistributed -- shapesOnDevice (a merge's recoded rows need only ``c`` and ``nCols``).
Their names are importable from here as before.
"""
import collections
import ctypes
import sys
import json
import os
import time

import numpy

from . import _lib
from . import shepseg
from . import tiling
# The jobs on the sharded output live in modules of their own; their names stay reachable here.
from .distdev import (idRange, spatialHaloPlan, disjointRowsError, _addr, deviceComm, Scratch, _raiseOnAllRanks,  # noqa: F401
                      _stepOnAllRanks, checkNpyOutfile, _overviewBlock, overviewPlan, _mosaicPieces, overviewTable,
                      overviewHoles)
from .dist_stats import (calcPerSegmentStatsDistributed, calcPerSegmentStatsDistributedBands, deviceStats,  # noqa: F401
                         deviceStatsBands, statsColumnsByName)
from .dist_spatial import (calcPerSegmentSpatialStatsDistributed, deviceSpatialStats, SEGPOINT_RECORD_BYTES,  # noqa: F401
                           userFuncRowPlan, clearUnownedRows, userFuncErrorOf)
from .dist_subset import subsetHeldRows, deviceSubset, subsetImageDistributed  # noqa: F401
from .dist_neighbours import (deviceNeighbours, findSegmentNeighboursDistributed, reduceOverNeighboursDistributed,  # noqa: F401
                              gatherSegmentNeighbours, mergeRule, deviceMerge, mergeSegmentsDistributed,
                              mergeSimilarSegmentsDistributed, aggregateToGroupsDistributed)
from .dist_colour import (RENDER_BLOCK_PIXELS, RENDER_GROUP_BLOCKS, colourShares, deviceColourTable,  # noqa: F401
                          writeColorTableFromRatColumnsDistributed, _NpyRgbaPatchWriter, deviceRender,
                          renderColourTableDistributed)
from .dist_shapes import SHAPE_RECORD_BYTES, deviceShapes, calcSegmentShapesDistributed  # noqa: F401


# ------------------------------------------------------------------------------------------
# sharding
# ------------------------------------------------------------------------------------------
def shardTileRows(tileInfo, world):
    """Contiguous blocks of tile rows per rank, balanced by pixel area.  Returns a list of
    (row0, row1) half-open ranges, one per rank (empty when there are more ranks than rows)."""
    nrows = tileInfo.nrows
    weights = []
    for r in range(nrows):
        weights.append(sum(tileInfo.getTile(c, r)[2] * tileInfo.getTile(c, r)[3]
                           for c in range(tileInfo.ncols)))
    total = float(sum(weights))
    out = []
    r = 0
    acc = 0.0
    for k in range(world):
        r0 = r
        remainingRanks = world - k
        if nrows - r <= 0:
            out.append((r, r))
            continue
        target = total * (k + 1) / world
        # take rows while it brings the running sum closer to this rank's share, keeping at
        # least one row for every later rank that can still get one
        while r < nrows and (nrows - r) > (remainingRanks - 1):
            if r > r0 and abs(acc + weights[r] - target) > abs(acc - target):
                break
            acc += weights[r]
            r += 1
        if r == r0 and r < nrows:
            acc += weights[r]
            r += 1
        out.append((r0, r))
    if r < nrows:                      # leftovers go to the last rank that has rows
        last = max(i for i, (a, b) in enumerate(out) if b > a)
        out[last] = (out[last][0], nrows)
    return out


def shardTiles(tileInfo, world, wholeRows=False):
    """Contiguous ranges [t0, t1) of tiles (row-major index row * ncols + col) per rank, balanced
    by pixel area.  Every rank that has a successor holds at least ncols tiles, so a tile's top
    neighbour is either local or in the previous rank; with fewer than ncols tiles per rank, or
    with wholeRows, the ranges are whole tile rows (shardTileRows), which has the same property.
    Whole rows are what the parallel stitch wants: a rank whose range starts in the middle of a
    tile row needs the right strip of the previous rank's LAST tile before its first chain step,
    whereas a row's first tile only needs the tile above it, which the previous rank stitches at
    the start of its last row -- the ranks then work one tile behind each other."""
    (ncols, nrows) = (tileInfo.ncols, tileInfo.nrows)
    nt = ncols * nrows
    if world <= 1:
        return [(0, nt)]
    if nt // world < ncols or wholeRows:
        return [(a * ncols, b * ncols) for (a, b) in shardTileRows(tileInfo, world)]
    weights = []
    for r in range(nrows):
        for c in range(ncols):
            (_x, _y, xs, ys) = tileInfo.getTile(c, r)
            weights.append(xs * ys)
    total = float(sum(weights))
    out = []
    i = 0
    acc = 0.0
    for k in range(world):
        i0 = i
        later = world - k - 1
        if k == world - 1:
            i = nt
        else:
            target = total * (k + 1) / world
            while i < nt - later * ncols:
                if i - i0 >= ncols and abs(acc + weights[i] - target) > abs(acc - target):
                    break
                acc += weights[i]
                i += 1
        out.append((i0, i))
    return out


def boundaryPlan(tileInfo, shards, p, overlapSize):
    """What rank p hands to the next rank that has tiles: a list of (kind, col, row, h, w) --
    'b' the recoded bottom strip (h x w) of a tile that is the top neighbour of one of the next
    rank's tiles, 'r' the right strip of rank p's last tile when the next rank starts in the
    middle of that tile row.  Both sides derive it from the shard table alone."""
    ncols = tileInfo.ncols
    nonEmpty = [i for i, (a, b) in enumerate(shards) if b > a]
    pos = nonEmpty.index(p)
    if pos + 1 >= len(nonEmpty):
        return []
    (p0, p1) = shards[p]
    (q0, q1) = shards[nonEmpty[pos + 1]]
    plan = []
    for t in range(max(p0, q0 - ncols), p1):
        if t + ncols < q1:                     # its bottom neighbour belongs to the next rank
            (col, row) = (t % ncols, t // ncols)
            (_x, _y, xs, ys) = tileInfo.getTile(col, row)
            plan.append(('b', col, row, min(overlapSize, ys), xs))
    if q0 % ncols != 0:
        (col, row) = ((p1 - 1) % ncols, (p1 - 1) // ncols)
        (_x, _y, xs, ys) = tileInfo.getTile(col, row)
        plan.append(('r', col, row, ys, min(overlapSize, xs)))
    return plan


def Comm(_unused=None, device=None):
    """World-size-1 communicator for callers that run the sharded driver in one process (kept as a
    public name: scripts and tests call it); multi-rank communicators come from pyshepseg_amd.comm."""
    from . import comm as _comm
    return _comm.LocalComm()


# ------------------------------------------------------------------------------------------
# the cross-tile stitch
# ------------------------------------------------------------------------------------------
# What the parallel form found: the final maxSegId `total` (every tile safe), `redoAll` (a tile outgrew
# the provisional id range) or a partial redo after tile `bad` (base: the final bases of all tiles,
# mAfter: the maxSegId after `bad`, fromPrev: the strips received with provisional ids)
ParallelOutcome = collections.namedtuple('ParallelOutcome', 'total redoAll bad base mAfter stride fromPrev',
                                         defaults=(None, False, None, None, None, None, None))


class _Stitch(object):
    """This rank's part of the stitch (the two forms of the module docstring).  The messages between
    ranks, in the order the communicators and both engines rely on -- sequential: maxSegId and the
    boundary strips from the previous rank, the chain, the same to the next rank, an all-gather of the
    final maxSegId; parallel: strips tile by tile in chain order, an all-gather of the tiles' counts,
    then nothing more, or the sequential form for all tiles or for the tiles after `bad` only."""

    def __init__(self, engine, comm, tileInfo, shards, jobs, overlap, simple, mark):
        (self.engine, self.comm, self.tileInfo, self.shards) = (engine, comm, tileInfo, shards)
        (self.jobs, self.overlap, self.simple, self.mark) = (jobs, overlap, simple, mark)
        self.jobmap = {(j.col, j.row): j for j in jobs}
        (self.t0, self.t1) = shards[comm.rank]
        self.ntAll = tileInfo.ncols * tileInfo.nrows
        self.nonEmpty = [i for i, (a, b) in enumerate(shards) if b > a]
        pos = self.nonEmpty.index(comm.rank) if jobs else -1
        self.prevRank = self.nonEmpty[pos - 1] if pos > 0 else None
        self.nextRank = self.nonEmpty[pos + 1] if jobs and pos + 1 < len(self.nonEmpty) else None

    def run(self, mode):
        """(maxSegId, stitch form, chain steps redone)"""
        if mode == 'sequential':
            return self.sequential(), mode, 0
        o = self.parallel()
        if o.redoAll:
            return self.sequential(), 'parallel->sequential', self.ntAll
        if o.bad is not None:
            return self.resume(o), 'parallel->sequential', self.ntAll - (o.bad + 1)
        return o.total, mode, 0

    def index(self, j):
        return j.row * self.tileInfo.ncols + j.col

    def winOf(self, j):
        return tiling.trimmedWindow(self.tileInfo, j.col, j.row, j.xpos, j.ypos, j.xsize, j.ysize, self.overlap)

    def neighbours(self, j, fromPrev):
        top = left = None
        if not self.simple:
            if j.row > 0:
                a = self.jobmap.get((j.col, j.row - 1))
                top = self.engine.bottomStripOf(a) if a is not None else fromPrev[('b', j.col, j.row - 1)]
            if j.col > 0:
                a = self.jobmap.get((j.col - 1, j.row))
                left = self.engine.rightStripOf(a) if a is not None else fromPrev[('r', j.col - 1, j.row)]
        return top, left

    def chain(self, jobs, maxSegId, fromPrev):
        """The sequential chain over `jobs`, numbering after maxSegId; returns the maxSegId after them."""
        self.engine.setMaxSegId(maxSegId)
        for j in jobs:
            self.engine.waitTile(j)
            (top, left) = self.neighbours(j, fromPrev)
            self.engine.stitchTile(j, top, left, self.winOf(j), self.simple)
        self.mark('chain issued')
        maxSegId = self.engine.getMaxSegId()
        self.mark('chain done')
        return maxSegId

    def receiveBoundary(self):
        """(maxSegId, strips) as the previous rank passed them on; (0, {}) on the first rank"""
        if self.prevRank is None:
            return 0, {}
        return self.engine.recvBoundary(self.comm, self.prevRank,
                                        boundaryPlan(self.tileInfo, self.shards, self.prevRank, self.overlap))

    def passOn(self, maxSegId):
        if self.nextRank is not None:
            plan = boundaryPlan(self.tileInfo, self.shards, self.comm.rank, self.overlap)
            self.engine.sendBoundary(self.comm, self.nextRank, maxSegId,
                                     [(kind, self.jobmap[(c, r)], h, w) for (kind, c, r, h, w) in plan])

    def finalMaxSegId(self, local):
        """the maxSegId of the last rank that has tiles, on every rank"""
        vals = self.comm.allgather_obj(int(local))
        return vals[self.nonEmpty[-1]] if self.nonEmpty else 0

    def sequential(self):
        maxSegId = 0
        if self.jobs:
            maxSegId = self.chain(self.jobs, *self.receiveBoundary())
            self.passOn(maxSegId)
        return self.finalMaxSegId(maxSegId)

    def parallel(self):
        (engine, comm, ntAll) = (self.engine, self.comm, self.ntAll)
        stride = 0xFFFFFFFF // max(ntAll, 1)
        (mine, fromPrev) = ([], {})
        if self.jobs:
            # With provisional ids a chain step needs its two neighbours only, so a rank takes its
            # tiles along anti-diagonals (row + col ascending): the tiles of its LAST row are then
            # done two steps apart instead of a row apart, and the next rank, which waits for them
            # one by one, follows two steps behind instead of a row behind.  Strips cross the rank
            # boundary tile by tile in that order ('b' before 'r'); both sides derive it.
            wave = os.environ.get('SHEPSEG_CHAIN_ORDER', 'diagonal') != 'rowmajor'
            tkey = (lambda c, r: (r + c, r)) if wave else (lambda c, r: (r * self.tileInfo.ncols + c, 0))

            def order(p):
                return sorted(boundaryPlan(self.tileInfo, self.shards, p, self.overlap),
                              key=lambda it: tkey(it[1], it[2]) + (it[0] != 'b',))
            planPrev = order(self.prevRank) if self.prevRank is not None else []
            sendOf = {}
            for it in (order(comm.rank) if self.nextRank is not None else []):
                sendOf.setdefault((it[1], it[2]), []).append(it)

            def need(key):
                while key not in fromPrev:
                    it = planPrev[len(fromPrev)]
                    fromPrev[it[:3]] = engine.recvStrip(comm, self.prevRank, it)
            engine.beginProvisional(stride, ntAll)
            for (slot, j) in sorted(enumerate(self.jobs), key=lambda sj: tkey(sj[1].col, sj[1].row)):
                if j.row > 0 and (j.col, j.row - 1) not in self.jobmap:
                    need(('b', j.col, j.row - 1))
                if j.col > 0 and (j.col - 1, j.row) not in self.jobmap:
                    need(('r', j.col - 1, j.row))
                engine.waitTile(j)
                (top, left) = self.neighbours(j, fromPrev)
                engine.stitchTileAt(j, top, left, self.winOf(j), self.index(j), stride, slot)
                for it in sendOf.get((j.col, j.row), ()):
                    engine.sendStrip(comm, self.nextRank, it, j)
            while len(fromPrev) < len(planPrev):          # (every planned strip has a reader; be safe)
                need(planPrev[len(fromPrev)][:3])
            if hasattr(engine, 'drainStrips'):
                engine.drainStrips()           # strips in flight must land before anything is renumbered
            counts = engine.tileCounts(len(self.jobs))
            mine = [(self.index(j), int(k), int(r), int(j.maxLocal)) for (j, (k, r)) in zip(self.jobs, counts)]
        everyone = [x for part in comm.allgather_obj(mine) for x in part]
        K = numpy.zeros(ntAll, dtype=numpy.int64)
        R = numpy.zeros(ntAll, dtype=numpy.int64)
        hard = len(everyone) != ntAll
        for (t, k, r, mloc) in everyone:
            K[t] = k
            R[t] = r
            if mloc >= stride or k >= stride:
                hard = True
        if hard or int(K.sum()) > 0xFFFFFFFF:
            return ParallelOutcome(redoAll=True)
        base = numpy.concatenate(([0], numpy.cumsum(K)[:-1])).astype(numpy.uint32)
        off = numpy.nonzero(K != R)[0]
        if len(off) == 0:
            if self.jobs:
                engine.renumber(stride, base)
            return ParallelOutcome(total=int(K.sum()))
        # Tile `bad` is the first (row-major) to hide ids it handed out from its trimmed window.  Up to
        # and including it the sequential run has maxSegId = sum of the earlier tiles' K at every step
        # (the induction of the safety test), so every decision taken so far -- bad's own recode
        # included -- stands and the provisional ids of tiles <= bad renumber to the final ones.  What
        # changes is where the NEXT tile starts: at base[bad] + R[bad], not + K[bad] (tiling.py:1029-1043:
        # maxSegId follows trimmed.max()).  The chain is redone from there only.
        bad = int(off[0])
        return ParallelOutcome(bad=bad, base=base, mAfter=int(base[bad]) + int(R[bad]), stride=stride,
                               fromPrev=fromPrev)

    def resume(self, o):
        """The partial redo: the tiles up to o.bad are kept, the chain runs again from o.bad + 1 on."""
        maxSegId = 0
        if self.jobs:
            kept = [j for j in self.jobs if self.index(j) <= o.bad]
            redo = [j for j in self.jobs if self.index(j) > o.bad]
            ownsBad = self.t0 <= o.bad < self.t1
            sendsOn = self.nextRank is not None and self.t1 - 1 >= o.bad     # (the next rank redoes all its tiles)
            # Final ids for what is kept, in each buffer that is read again: the output rows always (in
            # renumberKept); the kept tiles' strips when this rank redoes tiles or sends them on; the strips
            # that came from the previous rank with provisional ids on the rank that owns `bad` and redoes
            # tiles (a later rank receives its previous rank's strips again, with final ids).
            keptStripsReread = bool(redo) or sendsOn
            prevStripsReread = ownsBad and bool(redo)
            if kept:
                self.engine.renumberKept(o.stride, o.base, kept if keptStripsReread else [],
                                         list(o.fromPrev.values()) if prevStripsReread else [])
            if redo:
                maxSegId = self.chain(redo, *((o.mAfter, o.fromPrev) if ownsBad else self.receiveBoundary()))
            elif ownsBad:
                maxSegId = o.mAfter
            if sendsOn:
                self.passOn(maxSegId)
        return self.finalMaxSegId(maxSegId)


# ------------------------------------------------------------------------------------------
# the engine-agnostic driver
# ------------------------------------------------------------------------------------------
class DistResult(object):
    pass


def runDistributed(engine, comm, nRows, nCols, tileSize, overlapSize, minSegmentSize=50,
                   numClusters=60, subsamplePcnt=None, maxSpectralDiff='auto', imgNullVal=None,
                   fixedKMeansInit=True, fourConnected=True, simpleTileRecode=False,
                   spectDistPcntile=50, kmeansObj=None, stitchMode=None):
    """Tiled segmentation of an (nRows x nCols) raster, its tiles sharded over comm.world ranks.
    ``engine`` owns this rank's slice of the raster and of the output (the module docstring says
    what it provides; HipEngine).  Returns a
    DistResult with maxSegId, hist (global), kmeans, maxSpectralDiff, tileRange (row-major tile
    indices of this rank), rowRange (the tile rows they touch) and outRows (image rows of the
    output buffer this rank holds: its tiles' trimmed windows are written, the rest is 0) and
    stitchMode ('sequential', 'parallel', or 'parallel->sequential' when part of the parallel form
    had to be redone -- chainStepsRedone says how many tiles, from the first one whose ids the
    provisional numbering cannot express; argument / SHEPSEG_STITCH: None = parallel when
    comm.world > 1).  nRows, nCols, tileInfo and overlapSize describe the grid for the output stage
    (writeOutputDistributed)."""
    _t = [time.time()]
    _marks = []

    def _mark(what):                       # SHEPSEG_IO_TIMING: this rank's milestones of the step, to stderr at its end
        now = time.time()
        _marks.append('%s %.3f' % (what, now - _t[0]))
        _t[0] = now
    if stitchMode is None:
        stitchMode = os.environ.get('SHEPSEG_STITCH') or ('parallel' if comm.world > 1 else 'sequential')
    if stitchMode not in ('sequential', 'parallel'):
        raise ValueError("stitchMode must be 'sequential' or 'parallel'")
    if simpleTileRecode:
        stitchMode = 'sequential'          # (no shared segments: nothing to gain)
    if (overlapSize % 2) != 0:
        raise tiling.PyShepSegTilingError("Overlap size must be an even number")

    class _Ds(object):
        RasterXSize, RasterYSize = nCols, nRows
    tileInfo = tiling.getTilesForFile(_Ds(), tileSize, overlapSize)
    ncolsT = tileInfo.ncols
    shardBy = os.environ.get('SHEPSEG_SHARD') or ('rows' if stitchMode == 'parallel' else 'tiles')
    shards = shardTiles(tileInfo, comm.world, wholeRows=(shardBy == 'rows'))
    (t0, t1) = shards[comm.rank]
    jobs, total = tiling.makeTileJobs(tileInfo, tiles={(t % ncolsT, t // ncolsT) for t in range(t0, t1)})
    st = _Stitch(engine, comm, tileInfo, shards, jobs, overlapSize, simpleTileRecode, _mark)
    (r0, r1) = (t0 // ncolsT, (t1 - 1) // ncolsT + 1) if jobs else (0, 0)
    # image rows this rank needs (its tiles) and writes in the output (their trimmed windows)
    (yLo, yHi, outLo, outHi, sLo, sHi) = (0,) * 6
    if jobs:
        yLo = min(j.ypos for j in jobs)
        yHi = max(j.ypos + j.ysize for j in jobs)
        wins = [st.winOf(j) for j in jobs]
        outLo = min(w[5] for w in wins)
        outHi = max(w[5] + (w[1] - w[0]) for w in wins)
        # a disjoint split of the image rows for the k-means sample: from the first output row of this
        # rank's first tile to that of the next rank's first tile (inside both ranks' slices)
        def firstRow(p):
            (c, r) = (shards[p][0] % ncolsT, shards[p][0] // ncolsT)
            return tiling.trimmedWindow(tileInfo, c, r, *tileInfo.getTile(c, r), overlapSize)[5]
        sLo = 0 if st.prevRank is None else firstRow(comm.rank)
        sHi = nRows if st.nextRank is None else max(sLo, firstRow(st.nextRank))
    engine.setup(tileInfo, jobs, total, yLo, yHi, outLo, outHi, nCols, overlapSize)
    _mark('setup')

    # ---- one global k-means model (reference tiling.py:154-226) ----
    if kmeansObj is None:
        if subsamplePcnt is None:
            subsampleProp = min(1, numpy.sqrt(1000000 / (nRows * nCols)))
            subsamplePcnt = 100 * subsampleProp**2
        else:
            subsampleProp = numpy.sqrt(subsamplePcnt / 100.0)
        skip = int(round(1. / subsampleProp))
        ry = tiling._subsample_indices(nRows, skip)
        rx = tiling._subsample_indices(nCols, skip)
        mine = ry[(ry >= sLo) & (ry < sHi)]
        part = engine.subsample(mine, rx)                      # (nBands, len(mine), len(rx))
        parts = [p[0].reshape(p[1]) for p in comm.allgather_arrays(
            [numpy.ascontiguousarray(part), numpy.array(part.shape, dtype=numpy.int64)])]
        img = numpy.concatenate([p for p in parts if p.shape[1] > 0], axis=1)
        if (comm.world > 1 and getattr(comm, 'onDevice', False) and hasattr(comm, 'h') and fixedKMeansInit and
                hasattr(engine, 'fitSharded') and os.environ.get('SHEPSEG_FIT_SHARDED', '1') != '0'):
            # every rank holds the whole sample (12 MB for a 40000^2 raster); the E-step of the fit is sharded by
            # sample rows over the ranks, its labels all-gathered on the device every iteration, the M-step run by
            # all of them alike: the same model on every rank, no broadcast (shp_kmeans_fit_planar_dist)
            km = engine.fitSharded(img, numClusters, imgNullVal, comm)
            centres = numpy.ascontiguousarray(km.cluster_centers_, dtype=numpy.float64)
        else:
            centres = None
            if comm.rank == 0:
                km = engine.fit(img, numClusters, imgNullVal, fixedKMeansInit)
                centres = numpy.ascontiguousarray(km.cluster_centers_, dtype=numpy.float64)
            centres = comm.bcast_obj(centres, src=0)
        kmeansObj = shepseg.KMeansModel(centres)
    centres = numpy.ascontiguousarray(kmeansObj.cluster_centers_, dtype=numpy.float64)
    msd = shepseg.autoMaxSpectralDiff(kmeansObj, maxSpectralDiff, spectDistPcntile)

    # ---- segment this rank's tiles (asynchronously) ----
    _mark('model')
    engine.startSegmentation(centres, msd, imgNullVal, fourConnected, minSegmentSize)
    _mark('workers started')

    # ---- the stitch ----
    (maxSegId, stitchMode, chainRedone) = st.run(stitchMode)
    # A tile hands out at most one id per pixel, so no stitch ends above the tiles' total area.  Every rank
    # holds the same all-gathered value and raises alike, instead of sizing the histogram (and the all-reduce
    # that follows) by ids that are still provisional.
    maxPossible = sum(xs * ys for (_x, _y, xs, ys) in tileInfo.tiles.values())
    if not 0 <= maxSegId <= maxPossible:
        raise tiling.PyShepSegTilingError(
            "stitch ended with maxSegId %d, more than the %d pixels of all tiles (stitch form %s)"
            % (maxSegId, maxPossible, stitchMode))
    _mark('tiles + stitch')
    hist = engine.histogram(maxSegId) if jobs else numpy.zeros(maxSegId + 1, numpy.int64)
    hist = comm.allreduce_sum_i64(numpy.asarray(hist, dtype=numpy.int64)).astype(numpy.uint32)
    hist[0] = 0
    _mark('histogram')
    engine.finish()
    _mark('finish')
    if os.environ.get('SHEPSEG_IO_TIMING'):
        tm = getattr(engine, 'timings', None)
        sys.stderr.write('  [dist rank %d] %s%s\n' % (comm.rank, ', '.join(_marks),
                                                      ' | worker timers %s' % tm.makeSummaryDict() if tm is not None else ''))

    res = DistResult()
    res.maxSegId = int(maxSegId)
    res.hist = hist
    res.kmeans = kmeansObj
    res.maxSpectralDiff = msd
    res.stitchMode = stitchMode
    res.chainStepsRedone = chainRedone      # parallel form: tiles whose chain step ran a second time
    res.subsamplePcnt = subsamplePcnt
    res.rowRange = (r0, r1)
    res.tileRange = (t0, t1)
    res.outRows = (outLo, outHi)
    res.numTileRows, res.numTileCols = tileInfo.nrows, tileInfo.ncols
    res.hasEmptySegments = bool((hist[1:] == 0).any())
    (res.nRows, res.nCols, res.tileInfo, res.overlapSize) = (nRows, nCols, tileInfo, overlapSize)    # (the output stage)
    return res


# ------------------------------------------------------------------------------------------
# file to file: the slice reader, the overview ownership plan, the output stage
# ------------------------------------------------------------------------------------------
def readSlice(src, bandNumbers, yLo, yHi):
    """Rows [yLo, yHi) of the 1-based bands ``bandNumbers`` of a tiling._open_source source, as one
    C-contiguous (len(bandNumbers), yHi - yLo, nCols) array in a pixel type of the library, converted as
    _lib.as_image converts (int8 -> int16, 64-bit -> uint32 or int32 by the values of these rows; TypeError
    for anything else).  Reads those rows only (src.readRowsInto)."""
    bands = [int(b) - 1 for b in bandNumbers]
    out = numpy.empty((len(bands), int(yHi) - int(yLo), src.RasterXSize), dtype=src.dtype)
    if out.size:
        src.readRowsInto(bands, int(yLo), int(yHi), out)
    return _lib.as_image(out)[0]


class _NpyPatchWriter(tiling._NpyRowWriter):
    """An existing (nRows, nCols) uint32 .npy file (made by _NpyRowWriter) opened for pwrite by any rank."""
    def __init__(self, path, nrows, ncols):
        with open(path, 'rb') as f:
            version = numpy.lib.format.read_magic(f)
            (shape, fortran, dtype) = numpy.lib.format._read_array_header(f, version)
            self.offset = f.tell()
        if shape != (nrows, ncols) or fortran or dtype != numpy.dtype(numpy.uint32):
            raise tiling.PyShepSegTilingError("%s holds %s %s, not (%d, %d) uint32" % (path, shape, dtype, nrows, ncols))
        (self.nrows, self.ncols) = (nrows, ncols)
        self.fd = os.open(path, os.O_WRONLY)

    def writeRect(self, y0, x0, v):
        """v (h x w) at rows [y0, y0 + h), columns [x0, x0 + w): whole rows in one pwrite, else row by row"""
        (h, w) = v.shape
        if x0 == 0 and w == self.ncols:
            return self.writeRows(y0, y0 + h, v)
        for r in range(h):
            mv = memoryview(numpy.ascontiguousarray(v[r])).cast('B')
            pos = self.offset + ((y0 + r) * self.ncols + x0) * 4
            done = 0
            while done < len(mv):
                done += os.pwrite(self.fd, mv[done:], pos + done)


def writeOutputDistributed(engine, comm, dres, outfile, writeHistogram=True, timings=None):
    """The output stage of a multi-rank run, after runDistributed(engine, comm, ...) returned ``dres`` (every id
    final; the engine kept its output rows: outputRows, overviewRects).  Writes what the one-GPU driver writes
    for a .npy ``outfile`` (tiling.doTiledShepherdSegmentation): the mosaic, ``<base>_hist.npy`` (writeHistogram,
    rank 0) and ``<base>_ov<lvl>.npy`` for each level of tiling.overviewLevels -- rank 0 creates every file,
    zero-filled at full size, then each rank writes its own pixels with pwrite: its output rows in one piece
    when it holds whole tile rows, else its tiles' trimmed windows (SHEPSEG_SHARD=tiles: ranks share rows), and
    the overview pixels its tiles own (overviewPlan), sampled on the engine in one call.  Errors are raised on
    every rank.  ``timings`` (a tiling.Timers, optional) gets 'writing' and 'overviews'.  Returns the band
    statistics (tiling.estimateStatsFromHisto), the same on every rank."""
    Err = tiling.PyShepSegTilingError
    checkNpyOutfile(outfile)
    timings = timings if timings is not None else tiling.Timers()
    (nRows, nCols) = (dres.nRows, dres.nCols)
    base = outfile[:-4]
    layers = [(int(lvl), base + '_ov%d.npy' % lvl, ((nRows + lvl - 1) // lvl, (nCols + lvl - 1) // lvl))
              for lvl in tiling.overviewLevels(nCols, nRows)]

    def create():
        if comm.rank == 0:
            for (path, shape) in [(outfile, (nRows, nCols))] + [(p, s) for (_l, p, s) in layers]:
                tiling._NpyRowWriter(path, *shape).close()
            if writeHistogram:
                numpy.save(base + '_hist.npy', dres.hist)
    _stepOnAllRanks(comm, outfile, create, Err)

    def mosaic():
        pieces = _mosaicPieces(dres)
        if not pieces:
            return
        block = max(1, tiling.STREAM_BLOCK_ROWS)
        w = _NpyPatchWriter(outfile, nRows, nCols)
        try:
            (lo, hi) = dres.outRows
            for y in range(lo, hi, block):
                y1 = min(hi, y + block)
                rows = None
                for (a, b, x0, x1) in pieces:
                    (ra, rb) = (max(a, y), min(b, y1))
                    if ra < rb:
                        if rows is None:
                            rows = engine.outputRows(y, y1)
                        w.writeRect(ra, x0, rows[ra - y:rb - y, x0:x1])
        finally:
            w.close()
    with timings.interval('writing'):
        _stepOnAllRanks(comm, outfile, mosaic, Err)

    def overviews():
        (table, where, npacked) = overviewTable(dres, [lvl for (lvl, _p, _s) in layers])
        if not where:
            return
        packed = engine.overviewRects(table, npacked)
        files = {lvl: _NpyPatchWriter(path, *shape) for (lvl, path, shape) in layers}
        try:
            for (q, (lvl, x0, y0, x1, y1)) in zip(table, where):
                n = int(q[3] * q[4])
                files[lvl].writeRect(y0, x0, packed[q[5]:q[5] + n].reshape(y1 - y0, x1 - x0))
        finally:
            for f in files.values():
                f.close()
    if layers:
        with timings.interval('overviews'):
            _stepOnAllRanks(comm, base + '_ov*.npy', overviews, Err)
    hist = dres.hist
    if dres.hasEmptySegments and comm.rank == 0:
        tiling._warnEmptySegments(hist, dres.overlapSize)
    return tiling.estimateStatsFromHisto(hist) if hist.sum() > 0 else []


# ------------------------------------------------------------------------------------------
# HIP engine: this rank's GPU
# ------------------------------------------------------------------------------------------
class HipEngine(object):
    """Holds rows [yLo, yHi) of the raster in HBM (a DeviceRaster created by `makeSlice`),
    segments this rank's tiles with pooled worker contexts and stitches them on the device.
    Boundary strips go from this rank's strip block straight into ncclSend (RcclComm), or through
    host memory when the communicator is not on the device (SocketComm: ranks sharing a GPU)."""

    def __init__(self, makeSlice, numWorkers=16, keepOutput=False):
        self.makeSlice = makeSlice          # f(yLo, yHi) -> DeviceRaster of those rows
        self.numWorkers = numWorkers
        self.keepOutput = keepOutput
        self.ras = None
        self.timings = tiling.Timers()
        self._sliceKey = None

    def setup(self, tileInfo, jobs, total, yLo, yHi, outLo, outHi, nCols, overlapSize):
        self.c = _lib.chain_ctx()
        self.L = self.c._L
        self.tileInfo, self.jobs = tileInfo, jobs
        (self.yLo, self.yHi, self.outLo, self.outHi) = (yLo, yHi, outLo, outHi)
        self.nCols, self.overlap = nCols, overlapSize
        if self._sliceKey != (yLo, yHi):
            if self.ras is not None:
                self.ras.free()
            self.ras = self.makeSlice(yLo, yHi) if yHi > yLo else None
            self._sliceKey = (yLo, yHi)
        # other ranks' tiles share the output rows: what this rank does not write must read as null
        self.bufs = tiling._StitchBuffers(self.c, tileInfo, jobs, total, outLo, outHi, nCols, overlapSize,
                                          zeroOut=True)
        self.threads, self.forceExit = [], None
        self.recvDev = []

    def subsample(self, rowsGlobal, cols):
        nb = self.ras.shape[0] if self.ras is not None else 0
        if self.ras is None or len(rowsGlobal) == 0:
            return numpy.zeros((nb, 0, len(cols)), dtype=numpy.uint16)
        ry = (rowsGlobal - self.yLo).astype(numpy.uint32)
        out = numpy.empty((nb, len(ry), len(cols)), dtype=self.ras.dtype)
        self.c.check(self.L.shp_dev_subsample(
            self.c.handle, ctypes.c_void_p(self.ras.ptr), _lib.SHP_DTYPES[self.ras.dtype], nb,
            self.ras.shape[1], self.ras.shape[2], _lib.ptr(ry), len(ry),
            _lib.ptr(numpy.ascontiguousarray(cols, dtype=numpy.uint32)), len(cols), _lib.ptr(out)))
        return out

    def fit(self, img, numClusters, imgNullVal, fixedKMeansInit):
        with self.timings.interval('spectralclusters'):
            return shepseg.fitSpectralClusters(img, numClusters, 100, imgNullVal, fixedKMeansInit)

    def fitSharded(self, img, numClusters, imgNullVal, comm):
        with self.timings.interval('spectralclusters'):
            return shepseg.fitSpectralClusters(img, numClusters, 100, imgNullVal, True, _commHandle=comm.h)

    def startSegmentation(self, centres, msd, imgNullVal, fourConnected, minSegmentSize):
        if not self.jobs:
            return
        self.threads, self.forceExit = tiling.startSegmentationWorkers(
            self.ras, self.jobs, self.bufs.d_tiles, centres, msd, imgNullVal, fourConnected,
            minSegmentSize, self.numWorkers, self.timings, yOrigin=self.yLo,
            stitchPrep=(self.tileInfo, self.overlap, self.bufs.arena, False))

    def waitTile(self, j):
        tiling.waitForTile(j, self.jobs, self.threads, self.forceExit, 600)

    def setMaxSegId(self, v):
        a = numpy.array([v], dtype=numpy.uint32)
        self.c.check(self.L.shp_dev_upload(self.c.handle, self.bufs.d_scal, _lib.ptr(a), 4))

    def getMaxSegId(self):
        a = numpy.zeros(1, dtype=numpy.uint32)
        self.c.check(self.L.shp_sync(self.c.handle))
        self.c.check(self.L.shp_dev_download(self.c.handle, _lib.ptr(a), self.bufs.d_scal, 4))
        return int(a[0])

    # strips are (device pointer, row pitch in elements)
    def bottomStripOf(self, a):      # dense recoded strip written by the chain step of tile a
        return self.bufs.bottomStrip(a)

    def rightStripOf(self, a):
        return self.bufs.rightStrip(a)

    def stitchTile(self, j, top, left, win, simple):
        with self.timings.interval('stitchtiles'):
            self.bufs.step(j, top, left, win, simple)

    # ---- parallel stitch: provisional bases, per-tile counts, eager strips ----
    def beginProvisional(self, stride, ntAll):
        bases = (numpy.arange(ntAll, dtype=numpy.uint64) * stride).astype(numpy.uint32)
        self.nbBases = (ntAll + 2 * len(self.jobs) + 16) * 4
        self.d_bases = tiling._devAlloc(self.c, self.nbBases)
        self.c.check(self.L.shp_dev_memset(self.c.handle, self.d_bases, 0, self.nbBases))
        self.c.check(self.L.shp_dev_upload(self.c.handle, self.d_bases, _lib.ptr(bases), ntAll * 4))
        self.ntAll = ntAll

    def stitchTileAt(self, j, top, left, win, t, stride, slot):
        """The chain step of tile t with its provisional base (a device word of its own, so nothing
        is uploaded or read back per tile), then its two counts into slot `slot`."""
        with self.timings.interval('stitchtiles'):
            self.bufs.step(j, top, left, win, False, scalar=self.d_bases.value + 4 * t)
            self.c.check(self.L.shp_stitch_counts_dev(
                self.c.handle, ctypes.c_void_p(j.meta), j.maxLocal, (t * stride) & 0xFFFFFFFF,
                ctypes.c_void_p(self.d_bases.value + 4 * (self.ntAll + 2 * slot))))

    def tileCounts(self, n):
        a = numpy.zeros(2 * max(n, 1), dtype=numpy.uint32)
        self.c.check(self.L.shp_sync(self.c.handle))
        self.c.check(self.L.shp_dev_download(self.c.handle, _lib.ptr(a),
                                             ctypes.c_void_p(self.d_bases.value + 4 * self.ntAll), 8 * max(n, 1)))
        tiling._devRelease(self.c, self.d_bases, self.nbBases)
        self.d_bases = None
        return a[:2 * n].reshape(n, 2)

    def renumber(self, stride, base):
        self.c.check(self.L.shp_sync(self.c.handle))
        base = numpy.ascontiguousarray(base, dtype=numpy.uint32)
        self.c.check(self.L.shp_renumber_dev(self.c.handle, self.bufs.d_out, (self.outHi - self.outLo) * self.nCols,
                                             int(stride), _lib.ptr(base), len(base)))

    def renumberKept(self, stride, base, keptJobs, recvStrips):
        """provisional -> final ids in the output rows, in the recoded strips of the tiles that are kept
        and in EXACTLY the strips handed in (received from the previous rank with provisional ids: the
        partial redo of the parallel stitch) -- a buffer received with final ids must not be touched again."""
        self.renumber(stride, base)
        base = numpy.ascontiguousarray(base, dtype=numpy.uint32)

        def stripWords(j):
            return j.ysize * min(self.overlap, j.xsize) + min(self.overlap, j.ysize) * j.xsize      # right | bottom
        # the kept tiles' strips: runs of jobs whose strips are adjacent in the strip block go in one call
        runs = []
        for j in sorted(keptJobs, key=lambda q: q.rightOff):
            n = stripWords(j)
            if runs and runs[-1][0] + runs[-1][1] == j.rightOff:
                runs[-1][1] += n
            else:
                runs.append([j.rightOff, n])
        for (o, n) in runs:
            self.c.check(self.L.shp_renumber_dev(self.c.handle, ctypes.c_void_p(self.bufs.d_strips.value + 4 * o),
                                                 n, int(stride), _lib.ptr(base), len(base)))
        sizes = {d.value: nbytes for (d, nbytes) in self.recvDev}
        for (ptr, _w) in recvStrips:
            self.c.check(self.L.shp_renumber_dev(self.c.handle, ctypes.c_void_p(ptr), sizes[ptr] // 4, int(stride),
                                                 _lib.ptr(base), len(base)))

    def sendStrip(self, comm, dst, item, a):
        (kind, _c, _r, h, w) = item
        if hasattr(comm, 'isend_dev'):
            # asynchronous: the send waits ON THE DEVICE for the chain step that writes the strip, the chain
            # (this thread and its stream) goes on with the next tile
            (ptr, _pitch) = self.bottomStripOf(a) if kind == 'b' else self.rightStripOf(a)
            comm.isend_dev(ptr, h * w * 4, dst, self.c)
            self.asyncComm = comm
            return
        self.c.check(self.L.shp_sync(self.c.handle))          # the chain step that wrote it is done
        self._sendOne(comm, dst, kind, a, h * w)

    def recvStrip(self, comm, src, item):
        (kind, _c, _r, h, w) = item
        if hasattr(comm, 'irecv_dev'):
            d = tiling._devAlloc(self.c, h * w * 4)
            self.recvDev.append((d, h * w * 4))
            comm.irecv_dev(d.value, h * w * 4, src, self.c)     # the chain's stream waits for the data, not the host
            self.asyncComm = comm
            return (d.value, w)
        return (self._recvOne(comm, src, h * w), w)

    def drainStrips(self):
        """every strip sent or received asynchronously so far has arrived (host wait)"""
        c = getattr(self, 'asyncComm', None)
        if c is not None:
            c.drain()
            self.asyncComm = None

    def _sendOne(self, comm, dst, kind, a, n):
        (ptr, _pitch) = self.bottomStripOf(a) if kind == 'b' else self.rightStripOf(a)
        if comm.onDevice:        # device memory straight into RCCL
            comm.send_dev(ptr, n * 4, dst)
        else:                    # ranks without a device transport: stage through host memory
            buf = numpy.empty(n, dtype=numpy.uint32)
            self.c.check(self.L.shp_dev_download(self.c.handle, _lib.ptr(buf), ctypes.c_void_p(ptr), n * 4))
            comm.send_bytes(buf, dst)

    def _recvOne(self, comm, src, n):
        d = tiling._devAlloc(self.c, n * 4)
        self.recvDev.append((d, n * 4))
        if comm.onDevice:
            comm.recv_dev(d.value, n * 4, src)
        else:
            buf = numpy.frombuffer(comm.recv_bytes(src), dtype=numpy.uint32)
            self.c.check(self.L.shp_dev_upload(self.c.handle, d, _lib.ptr(numpy.ascontiguousarray(buf)), n * 4))
        return d.value

    def sendBoundary(self, comm, dst, maxSegId, items):
        """items: (kind, job, h, w) from boundaryPlan; strips are dense h x w blocks."""
        self.c.check(self.L.shp_sync(self.c.handle))
        comm.send_obj(int(maxSegId), dst)
        for (kind, a, h, w) in items:
            self._sendOne(comm, dst, kind, a, h * w)

    def recvBoundary(self, comm, src, plan):
        maxSegId = int(comm.recv_obj(src))
        strips = {}
        for (kind, col, row, h, w) in plan:
            strips[(kind, col, row)] = (self._recvOne(comm, src, h * w), w)
        return maxSegId, strips

    def histogram(self, maxSegId):
        hist = numpy.zeros(maxSegId + 1, dtype=numpy.uint32)
        self.c.check(self.L.shp_histogram_dev(self.c.handle, self.bufs.d_out,
                                              (self.outHi - self.outLo) * self.nCols, self.nCols, maxSegId,
                                              _lib.ptr(hist)))
        return hist

    def _heldOut(self):
        """Device address of this rank's rows of the kept output; 0 when it holds none."""
        return _addr(self._lastOut) if self.outHi > self.outLo else 0

    def _bandPtr(self, imgbandnum):
        """Device address of this rank's OUTPUT rows of one image band (1-based band number)."""
        (nb, rows, cols) = self.ras.shape
        isz = numpy.dtype(self.ras.dtype).itemsize
        return self.ras.ptr + (((imgbandnum - 1) * rows + (self.outLo - self.yLo)) * cols) * isz

    # ---- the split of the per-segment statistics (_distributedStats: the ...Bands set of methods)
    @property
    def numBands(self):
        """image bands this rank holds rows of (None: no rows, so it cannot tell)"""
        return self.ras.shape[0] if self.ras is not None else None

    def _bandPointers(self, bandNums):
        arr = (ctypes.c_void_p * len(bandNums))()
        for (k, b) in enumerate(bandNums):
            arr[k] = self._bandPtr(b)
        return arr

    def localStatsBands(self, bandNums, S, fast, perBand, nInt, nFloat, missing, nullVals):
        """all entries' columns over this rank's output rows, in one pass over the labels (shp_segstats2d_bands_dev)"""
        nRows = self.outHi - self.outLo
        ic = numpy.zeros((max(nInt, 1), S + 1), dtype=numpy.int64)
        fc = numpy.zeros((max(nFloat, 1), S + 1), dtype=numpy.float32)
        if nRows * self.nCols > 0:
            hasNull = numpy.ascontiguousarray([int(v is not None) for v in nullVals], dtype=numpy.int32)
            nullArr = numpy.ascontiguousarray([0 if v is None else int(v) for v in nullVals], dtype=numpy.int64)
            self.c.check(self.L.shp_segstats2d_bands_dev(
                self.c.handle, self._lastOut, self._bandPointers(bandNums), _lib.SHP_DTYPES[self.ras.dtype], len(bandNums),
                nRows, self.nCols, S, _lib.ptr(hasNull), _lib.ptr(nullArr), _lib.ptr(fast), _lib.ptr(perBand), int(missing),
                _lib.ptr(ic), _lib.ptr(fc)))
        return ic[:nInt], fc[:nFloat]

    def gatherFlaggedBands(self, planes, S, flags, count):
        """the pixels of the flagged ids in this rank's output rows: the ids once and (len(planes), count) values in
        the image's pixel type, every row in the order of the ids (shp_gather_flagged_bands_dev)"""
        n = (self.outHi - self.outLo) * self.nCols
        dt = self.ras.dtype if self.ras is not None else numpy.dtype(numpy.uint16)
        segs = numpy.empty(max(count, 1), dtype=numpy.uint32)
        vals = numpy.empty((len(planes), max(count, 1)), dtype=numpy.int64)
        got = ctypes.c_int64(0)
        if n > 0 and count > 0:
            self.c.check(self.L.shp_gather_flagged_bands_dev(
                self.c.handle, self._lastOut, self._bandPointers(planes), _lib.SHP_DTYPES[self.ras.dtype], len(planes), n, S,
                _lib.ptr(flags), count, _lib.ptr(segs), _lib.ptr(vals), ctypes.byref(got)))
            if got.value != count:
                raise tiling.PyShepSegTilingError(
                    "straddling-segment gather found %d pixels, histogram says %d" % (got.value, count))
        return segs[:count], vals[:, :count].astype(dt)

    def statsOfPairsBands(self, segs, vals, K, planeOfEntry, fast, perBand, nInt, nFloat, missing, nullVals):
        """the entries' columns of a list of pairs: ``vals`` one array per distinct band in the order of ``segs``
        (compact ids 1..K), entry e reads vals[planeOfEntry[e]] -- the bands kernels on a 1 x M raster."""
        m = len(segs)
        dt = numpy.dtype(self.ras.dtype if self.ras is not None else vals[0].dtype)
        ic = numpy.zeros((max(nInt, 1), K + 1), dtype=numpy.int64)
        fc = numpy.zeros((max(nFloat, 1), K + 1), dtype=numpy.float32)
        rowBytes = (m * dt.itemsize + 15) // 16 * 16
        with Scratch(self.c) as s:
            blocks = [s.alloc(sz) for sz in [m * 4] + [rowBytes] * len(vals)]
            segs = numpy.ascontiguousarray(segs, dtype=numpy.uint32)
            self.c.check(self.L.shp_dev_upload(self.c.handle, blocks[0], _lib.ptr(segs), m * 4))
            for (k, v) in enumerate(vals):
                v = numpy.ascontiguousarray(v).astype(dt, copy=False)
                self.c.check(self.L.shp_dev_upload(self.c.handle, blocks[1 + k], _lib.ptr(v), m * dt.itemsize))
            ptrs = (ctypes.c_void_p * len(planeOfEntry))(*[blocks[1 + p].value for p in planeOfEntry])
            hasNull = numpy.ascontiguousarray([int(v is not None) for v in nullVals], dtype=numpy.int32)
            nullArr = numpy.ascontiguousarray([0 if v is None else int(v) for v in nullVals], dtype=numpy.int64)
            self.c.check(self.L.shp_segstats2d_bands_dev(
                self.c.handle, blocks[0], ptrs, _lib.SHP_DTYPES[dt], len(planeOfEntry), 1, m, K, _lib.ptr(hasNull),
                _lib.ptr(nullArr), _lib.ptr(fast), _lib.ptr(perBand), int(missing), _lib.ptr(ic), _lib.ptr(fc)))
        return ic[:nInt], fc[:nFloat]

    def statsBandsOnDevice(self, comm, hist, planes, planeOfEntry, fast, perBand, nullVals, nInt, nFloat, missing):
        """calcPerSegmentStatsDistributed[Bands]' device path for this rank's output rows (deviceStatsBands).
        planes: the distinct band numbers, planeOfEntry[e]: which of them entry e reads."""
        held = self.ras is not None and self.outHi > self.outLo
        if held:
            d_out = _addr(self._lastOut)
            d_planes = [self._bandPtr(b) for b in planes]
            dtypeCode = _lib.SHP_DTYPES[self.ras.dtype]
        else:
            # (no rows: nothing is read; the addresses only say which entries share a band, and the pixel type, which
            #  sizes this rank's empty block of the exchange, is taken from the other ranks)
            (d_out, d_planes, dtypeCode) = (0, [16 * (p + 1) for p in range(len(planes))], None)
        hasNull = [int(v is not None) for v in nullVals]
        nullArr = [0 if v is None else int(v) for v in nullVals]
        return deviceStatsBands(self.c, comm, d_out, [d_planes[p] for p in planeOfEntry], dtypeCode,
                                (self.outHi - self.outLo) if held else 0, self.nCols, hist, fast, perBand, hasNull, nullArr,
                                nInt, nFloat, missing)

    def spatialOnDevice(self, comm, hist, imgbandnum, colTypes, userFunc, userParam, missing, imgNullVal,
                        tileSize=tiling.TILESIZE, batchPoints=None, info=None):
        """calcPerSegmentSpatialStatsDistributed's path for this rank's output rows (deviceSpatialStats)."""
        d_out = self._heldOut()
        return deviceSpatialStats(self.c, comm, d_out, self._bandPtr(imgbandnum) if d_out else 0,
                                  _lib.SHP_DTYPES[self.ras.dtype] if self.ras is not None else -1, None, self.nCols,
                                  (self.outLo, self.outHi), hist, colTypes, userFunc, userParam, missing, imgNullVal,
                                  tileSize=tileSize, batchPoints=batchPoints, info=info)

    def subsetOnDevice(self, comm, maxSegId, tlx, tly, xs, ys, mask=None, tileSize=None):
        """subsetImageDistributed's path for this rank's output rows (deviceSubset)."""
        return deviceSubset(self.c, comm, self._heldOut(), None, self.nCols, (self.outLo, self.outHi), maxSegId, tlx, tly, xs,
                            ys, mask=mask, tileSize=tileSize)

    def neighboursOnDevice(self, comm, maxSegId, fourConnected=True, info=None):
        """findSegmentNeighboursDistributed's path for this rank's output rows (deviceNeighbours)."""
        return deviceNeighbours(self.c, comm, self._heldOut(), None, self.nCols, (self.outLo, self.outHi), maxSegId,
                                fourConnected=fourConnected, info=info)

    def shapesOnDevice(self, comm, maxSegId, hist, missingStatsValue=-9999, info=None):
        """calcSegmentShapesDistributed's path for this rank's output rows (deviceShapes)."""
        return deviceShapes(self.c, comm, self._heldOut(), None, self.nCols, (self.outLo, self.outHi), maxSegId, hist,
                            missingStatsValue=missingStatsValue, info=info)

    def mergeOnDevice(self, comm, share, rule, nRows, outfile=None, info=None):
        """mergeSegmentsDistributed's path with this rank's output rows recoded (deviceMerge)."""
        return deviceMerge(self.c, comm, share, rule, self._heldOut(), nRows, self.nCols, (self.outLo, self.outHi), outfile=outfile,
                           info=info)

    def localOutput(self):
        out = numpy.empty((self.outHi - self.outLo, self.nCols), dtype=numpy.uint32)
        self.c.check(self.L.shp_dev_download(self.c.handle, _lib.ptr(out), self._lastOut, out.nbytes))
        return out

    def outputRows(self, y0, y1):
        """image rows [y0, y1) of the kept output (inside outRows), to the host"""
        out = numpy.empty((y1 - y0, self.nCols), dtype=numpy.uint32)
        if out.size:
            self.c.check(self.L.shp_dev_download(self.c.handle, _lib.ptr(out),
                                                 ctypes.c_void_p(_addr(self._lastOut) + (y0 - self.outLo) * self.nCols * 4), out.nbytes))
        return out

    def overviewRects(self, table, npacked):
        """the overview rectangles of a writeOutputDistributed table sampled from the kept output in one launch
        (shp_overview_rects_dev), downloaded once: uint32 (npacked,)"""
        out = numpy.empty(npacked, dtype=numpy.uint32)
        if npacked == 0:
            return out
        table = numpy.ascontiguousarray(table, dtype=numpy.int64)
        with Scratch(self.c) as s:
            d = s.alloc(npacked * 4)
            self.c.check(self.L.shp_overview_rects_dev(self.c.handle, self._lastOut,
                                                       (self.outHi - self.outLo) * self.nCols, _lib.ptr(table),
                                                       table.shape[0], d, npacked))
            self.c.check(self.L.shp_dev_download(self.c.handle, _lib.ptr(out), d, out.nbytes))
        return out

    def colourTableOnDevice(self, comm, cols, info=None):
        """writeColorTableFromRatColumnsDistributed's path on this rank's GPU (deviceColourTable); the packed
        table stays here as ``colourTable`` = (device pointer, rows) until freeColourTable / releaseOutput"""
        self.freeColourTable()
        (columns, stretch, deviceMs, d_table, n) = deviceColourTable(self.c, comm, cols, info=info)
        self.colourTable = (d_table, n)
        return columns, stretch, deviceMs

    def colourTableRow(self, i):
        """row i of ``colourTable`` as (R, G, B, A) uint8"""
        row = numpy.zeros(4, dtype=numpy.uint8)
        self.c.check(self.L.shp_dev_download(self.c.handle, _lib.ptr(row),
                                             ctypes.c_void_p(_addr(self.colourTable[0]) + 4 * int(i)), 4))
        return row

    def freeColourTable(self):
        t = getattr(self, 'colourTable', None)
        if t is not None:
            tiling._devRelease(self.c, t[0], t[1] * 4)
        self.colourTable = None

    def renderOnDevice(self, comm, cols=None, rects=None, npacked=0, sink=None, blockPixels=None, info=None):
        """renderColourTableDistributed's path for this rank's output rows (deviceRender).  cols: the four byte
        columns of a table to upload for this call (shp_colour_pack), None: ``colourTable``."""
        held = self.outHi > self.outLo
        with Scratch(self.c) as s:
            table = getattr(self, 'colourTable', None)
            if cols is not None:
                table = (s.alloc(len(cols[0]) * 4), len(cols[0]))
                self.c.check(self.L.shp_colour_pack(self.c.handle, _lib.ptr(cols[0]), _lib.ptr(cols[1]),
                                                    _lib.ptr(cols[2]), _lib.ptr(cols[3]), table[1], table[0]))
            return deviceRender(self.c, comm, self._heldOut(), (self.outHi - self.outLo) if held else 0, self.nCols, table[0],
                                table[1], rects=rects, npacked=npacked, sink=sink, blockPixels=blockPixels, info=info)

    def finish(self):
        for t in self.threads:
            t.join()
        self.drainStrips()
        self.c.check(self.L.shp_sync(self.c.handle))
        for (d, nbytes) in self.recvDev:
            tiling._devRelease(self.c, d, nbytes)
        self.recvDev = []
        self.bufs.release(keepOut=self.keepOutput)
        if self.keepOutput:
            self._lastOut = self.bufs.d_out          # caller must releaseOutput()

    def releaseOutput(self):
        self.freeColourTable()
        tiling._devRelease(self.c, self.bufs.d_out, self.bufs.nbOut)


class _FileSliceEngine(HipEngine):
    """HipEngine whose makeSlice uploads rows [yLo, yHi) of the selected bands of a raster source (readSlice).
    The rows are read in setup, before any collective of runDistributed; what fails there (a 64-bit band
    outside the 32-bit range, a read error) is all-gathered and raised alike on every rank.  The output is
    always kept: writeOutputDistributed reads it; release() frees what the run left on the device."""

    def __init__(self, comm, src, bandNumbers, nullVal, numWorkers):
        HipEngine.__init__(self, self._upload, numWorkers=numWorkers, keepOutput=True)
        (self.comm, self.src, self.bandNumbers, self.nullVal) = (comm, src, bandNumbers, nullVal)
        (self._host, self._finished) = (None, False)
        (self.threads, self.forceExit) = ([], None)

    def _upload(self, yLo, yHi):
        with self.timings.interval('reading'):
            ras = tiling.DeviceRaster.fromArray(self._host, self.nullVal)
        self._host = None
        return ras

    def setup(self, tileInfo, jobs, total, yLo, yHi, outLo, outHi, nCols, overlapSize):
        err = None
        with self.timings.interval('reading'):
            try:
                if yHi > yLo:
                    self._host = readSlice(self.src, self.bandNumbers, yLo, yHi)
            except Exception as e:      # noqa: B902  (raised below, on every rank)
                err = e
        _raiseOnAllRanks(self.comm, err)
        HipEngine.setup(self, tileInfo, jobs, total, yLo, yHi, outLo, outHi, nCols, overlapSize)

    def finish(self):
        HipEngine.finish(self)
        self._finished = True

    def release(self):
        """Free every device block of the run: after a failure too (the workers are stopped first, and a buffer a
        worker may still write is leaked rather than reused, as in tiling.doTiledShepherdSegmentation)."""
        if self.forceExit is not None:
            self.forceExit.set()
        stuck = False
        for t in self.threads:
            t.join(timeout=None if self._finished else 120.0)
            stuck = stuck or t.is_alive()
        if getattr(self, 'c', None) is not None:
            self.L.shp_sync(self.c.handle)
        if stuck:
            sys.stderr.write("pyshepseg_amd: a worker did not stop after a failure; its device buffers are leaked "
                             "rather than reused\n")
            return
        if getattr(self, 'c', None) is not None:
            self.freeColourTable()
        if self._finished:
            if getattr(self, '_lastOut', None) is not None:
                self.releaseOutput()
                self._lastOut = None
        elif getattr(self, 'bufs', None) is not None:
            for (d, nbytes) in self.recvDev:
                tiling._devRelease(self.c, d, nbytes)
            self.recvDev = []
            if getattr(self, 'd_bases', None) is not None:
                tiling._devRelease(self.c, self.d_bases, self.nbBases)
                self.d_bases = None
            self.bufs.free()            # (a failed run: freed, not recycled)
        self.bufs = None
        if self.ras is not None:
            self.ras.free()
            self.ras = None
        self._sliceKey = None


def doTiledShepherdSegmentationDistributed(infile, outfile, comm=None, tileSize=tiling.DFLT_TILESIZE,
        overlapSize=tiling.DFLT_OVERLAPSIZE, minSegmentSize=50, numClusters=60, bandNumbers=None,
        subsamplePcnt=None, maxSpectralDiff='auto', imgNullVal=None, fixedKMeansInit=False,
        fourConnected=True, verbose=False, simpleTileRecode=False, spectDistPcntile=50, kmeansObj=None,
        writeHistogram=True, concurrencyCfg=None, stitchMode=None, keepOutput=False):
    """tiling.doTiledShepherdSegmentation from a raster file to a .npy file over the ranks of ``comm``: every
    rank calls it with the same arguments.  Each rank reads the rows its tiles need (readSlice) into its own
    GPU, runDistributed segments and stitches them, writeOutputDistributed writes the mosaic, the histogram
    and the overview layers -- the files the one-GPU driver writes, bit for bit.

    ``infile``: a numpy array, a .npy path or a GDAL-readable path (not a DeviceRaster); ``outfile``: a .npy
    path on a filesystem every rank sees (anything else raises tiling.PyShepSegTilingError on every rank before
    any collective, and creates nothing).  The segmentation keywords and their defaults are those of
    tiling.doTiledShepherdSegmentation; concurrencyCfg.numWorkers sizes the HipEngine; ``stitchMode`` as in
    runDistributed.  ``comm`` None: comm.fromEnvironment(), closed before returning (a communicator passed in
    stays open).  Argument errors (outfile, odd overlap, band numbers, pixel type) are raised alike on every
    rank.

    Returns a tiling.TiledSegmentationResult, the same on every rank: the fields of the one-GPU .npy path
    (segimg and overviews None: the layers are in the files), plus rowRange, outRows, tileRange, stitchMode and
    chainStepsRedone of the DistResult.  keepOutput=True: the raster slice and the labels stay on this rank's
    GPU, ``result.engine`` and ``result.dist`` (the DistResult) are set for calcPerSegmentStatsDistributed,
    calcPerSegmentSpatialStatsDistributed and subsetImageDistributed -- whose ``imgbandnum`` is the 1-based
    position of the band in ``bandNumbers`` when bands were selected -- and the caller frees them with
    result.engine.release().  keepOutput=False: every device block of the call is released, also on failure."""
    from . import comm as _comm
    Err = tiling.PyShepSegTilingError
    checkNpyOutfile(outfile)
    if isinstance(infile, tiling.DeviceRaster):
        raise Err("the multi-rank driver reads a numpy array, a .npy path or a GDAL raster, not a DeviceRaster "
                  "(it lives on one GPU)")
    if concurrencyCfg is None:
        concurrencyCfg = tiling.SegmentationConcurrencyConfig()
    numWorkers = 1
    if concurrencyCfg.concurrencyType != tiling.CONC_NONE:
        numWorkers = max(1, int(concurrencyCfg.numWorkers))
    ownComm = comm is None
    if ownComm:
        comm = _comm.fromEnvironment()
    engine = None
    ok = False
    try:
        timings = tiling.Timers()
        with timings.interval('walltime'):
            # ---- arguments: checked on every rank, the first rank's error raised on all of them
            err = src = None
            try:
                if (overlapSize % 2) != 0:
                    raise Err("Overlap size must be an even number")
                src = tiling._open_source(infile)
                nBandsAll = src.shape[0]
                if bandNumbers is None:
                    bandNumbers = list(range(1, nBandsAll + 1))
                bandNumbers = [int(b) for b in bandNumbers]
                if not bandNumbers or any(b < 1 or b > nBandsAll for b in bandNumbers):
                    raise Err("band numbers %s out of range 1..%d" % (bandNumbers, nBandsAll))
                _lib.as_image(numpy.zeros((1, 1, 1), dtype=src.dtype))        # (the pixel types as_image takes)
                if imgNullVal is None:
                    imgNullVal = (src.bandNull(bandNumbers) if isinstance(src, tiling._GdalSource)
                                  else src.nullVal)
            except Exception as e:      # noqa: B902  (raised below, on every rank)
                err = e
            _raiseOnAllRanks(comm, err)
            (nRows, nCols) = (src.RasterYSize, src.RasterXSize)
            engine = _FileSliceEngine(comm, src, bandNumbers, imgNullVal, numWorkers)
            dres = runDistributed(engine, comm, nRows, nCols, tileSize, overlapSize, minSegmentSize=minSegmentSize,
                                  numClusters=numClusters, subsamplePcnt=subsamplePcnt,
                                  maxSpectralDiff=maxSpectralDiff, imgNullVal=imgNullVal,
                                  fixedKMeansInit=fixedKMeansInit, fourConnected=fourConnected,
                                  simpleTileRecode=simpleTileRecode, spectDistPcntile=spectDistPcntile,
                                  kmeansObj=kmeansObj, stitchMode=stitchMode)
            if verbose and comm.rank == 0:
                print("KMeans of whole raster", dres.kmeans.n_clusters, "clusters; maxSpectralDiff",
                      dres.maxSpectralDiff)
                print("Found {} tiles, with {} rows and {} cols".format(
                    dres.numTileRows * dres.numTileCols, dres.numTileRows, dres.numTileCols))
            bandStatistics = writeOutputDistributed(engine, comm, dres, outfile, writeHistogram, timings=timings)
        for (name, pairs) in engine.timings.pairs.items():
            timings.pairs.setdefault(name, []).extend(pairs)
        result = tiling.TiledSegmentationResult()
        for k in ('maxSegId', 'hist', 'kmeans', 'maxSpectralDiff', 'subsamplePcnt', 'numTileRows', 'numTileCols',
                  'hasEmptySegments', 'rowRange', 'outRows', 'tileRange', 'stitchMode', 'chainStepsRedone'):
            setattr(result, k, getattr(dres, k))
        (result.bandStatistics, result.timings) = (bandStatistics, timings)
        (result.segimg, result.overviews) = (None, None)
        if keepOutput:
            (result.engine, result.dist) = (engine, dres)
        ok = True
        return result
    finally:
        if engine is not None and not (ok and keepOutput):
            engine.release()
        if ownComm:
            comm.close()


# ------------------------------------------------------------------------------------------
# bench.py entry for --gpus N > 1
# ------------------------------------------------------------------------------------------
def bench_stats_main(args, rank, world, local_rank):
    """One rank of `bench.py --workload c5 --gpus N`: the label raster of 4 x 8-pixel blocks (50 M segments at
    40000^2) and one uint16 band, sharded by rows at boundaries that CUT blocks (every shard boundary makes
    nCols / 8 straddling segments); a step = calcPerSegmentStatsDistributed's device path (deviceStats: one entry
    through deviceStatsBands, the driver of any number of entries), the assembled columns copied to the host on
    rank 0."""
    from . import comm as _comm
    from . import tilingstats
    comm = _comm.fromEnvironment()
    c = _lib.ctx()
    L = c._L
    dcomm = deviceComm(comm, c)
    (N, BH, BW) = (args.size, 4, 8)
    # shard boundaries two rows into a block row
    cuts = [0] + [min(N, ((N * (r + 1)) // world) // BH * BH + 2) for r in range(world - 1)] + [N]
    (y0, y1) = (cuts[rank], cuts[rank + 1])
    ras = tiling.DeviceRaster.synth(getattr(args, 'seed', 11), 1, y1 - y0, N, y0=y0, x0=0)
    d_full = ctypes.c_void_p()
    c.check(L.shp_dev_alloc(c.handle, N * N * 4, ctypes.byref(d_full)))
    S = ctypes.c_uint32(0)
    c.check(L.shp_dev_block_labels(c.handle, N, N, BH, BW, d_full, ctypes.byref(S)))
    S = S.value
    d_seg = d_full.value + y0 * N * 4                       # this rank's rows of the label raster
    h = numpy.full(S + 1, BH * BW, dtype=numpy.uint32)      # every block whole: the RAT's Histogram column
    h[0] = 0
    d_hist = ctypes.c_void_p()
    c.check(L.shp_dev_alloc(c.handle, h.nbytes, ctypes.byref(d_hist)))
    c.check(L.shp_dev_upload(c.handle, d_hist, _lib.ptr(h), h.nbytes))
    sel = [('mean', 'mean'), ('sd', 'stddev'), ('med', 'median'), ('n', 'pixcount')]
    (fast, nInt, nFloat) = tilingstats.makeFastStatsSelection(list(range(len(sel))), sel)

    def step():
        return deviceStats(c, dcomm, d_seg, ras.ptr, 2, y1 - y0, N, ('dev', d_hist.value, S + 1), fast, nInt, nFloat,
                           -9999, None, fetch=(rank == 0))

    for _ in range(args.warmup):
        res = step()
    c.check(L.shp_sync(c.handle))
    comm.barrier()
    t0 = time.time()
    for _ in range(args.steps):
        res = step()
    c.check(L.shp_sync(c.handle))
    comm.barrier()
    dt = comm.max_f64((time.time() - t0) / max(args.steps, 1))
    rcclRanks = comm.count() if hasattr(comm, 'count') else None
    if rank == 0:
        (ic, fc, nStrad, nPix) = res
        assert int(ic[fast[3, 3]].sum()) == N * N and (ic[fast[3, 3]][1:] == BH * BW).all()
        npix = N * N
        alg = 6 * npix + 4 * len(sel) * (S + 1)            # 6 B/px + 4 * nCols B/segment
        out = {
            "metric": "Mpixels/sec, tilingstats per-segment mean/stddev/median/pixcount",
            "value": round(npix / dt / 1e6, 3), "unit": "Mpixels/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt * 1e3, 2), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "u16", "data": "synthetic",
            "config": {"workload": "C5: %dx%d label raster of %d x %d-pixel blocks (%d segments) + one uint16 synthimg v1 "
                                   "band, rows sharded over %d GPUs at boundaries that cut blocks; 4 result columns "
                                   "assembled by one all-reduce and copied to the host on rank 0" % (N, N, BH, BW, S, world),
                       "segments": S, "straddlers": int(nStrad), "straddler_pixels": int(nPix),
                       "rows_per_rank": [cuts[r + 1] - cuts[r] for r in range(world)],
                       "transport": getattr(dcomm, 'transport', type(dcomm).__name__), "rccl_nranks": rcclRanks,
                       "parallelism": "label rows sharded over %d ranks, one process per GPU; straddling segments' pixels "
                                      "all-gathered as packed device buffers and reduced by id share; columns all-reduced" % world},
            "roofline": {"bound": "hbm", "kernel": "whole call (local statistics + exchange + all-reduce + download)",
                         "achieved": round(alg / dt / 1e9, 3), "peak": 8000.0 * world, "unit": "GB/s",
                         "frac": round(alg / dt / 1e9 / (8000.0 * world), 6), "traffic": None},
        }
        print(json.dumps(out), flush=True)
    comm.barrier()
    c.check(L.shp_dev_free(c.handle, d_hist))
    c.check(L.shp_dev_free(c.handle, d_full))
    ras.free()
    comm.close()


def bench_main(args, rank, world, local_rank):
    """One rank of the multi-GPU benchmark: this rank's rows of the synthetic image are generated
    in its own HBM (synthimg is position-deterministic); a step = runDistributed."""
    from . import comm as _comm
    comm = _comm.fromEnvironment()
    nb = args.bands

    def makeSlice(yLo, yHi):
        return tiling.DeviceRaster.synth(getattr(args, 'seed', 11), nb, yHi - yLo, args.size, y0=yLo, x0=0)
    engine = HipEngine(makeSlice, numWorkers=args.workers)
    sync = _lib.ctx()

    def step():
        return runDistributed(engine, comm, args.size, args.size, args.tile, args.overlap,
                              minSegmentSize=50, numClusters=60, fixedKMeansInit=True)

    for _ in range(args.warmup):
        r = step()
    sync.check(sync._L.shp_sync(sync.handle))
    comm.barrier()
    t0 = time.time()
    for _ in range(args.steps):
        r = step()
    sync.check(sync._L.shp_sync(sync.handle))
    comm.barrier()
    dt = comm.max_f64((time.time() - t0) / max(args.steps, 1))
    tilesPerRank = [int(x) for x in comm.allgather_obj(int(r.tileRange[1] - r.tileRange[0]))]
    rcclRanks = comm.count() if hasattr(comm, 'count') else None      # what RCCL itself says (ncclCommCount)
    fitShardedHere = (world > 1 and getattr(comm, 'onDevice', False) and hasattr(comm, 'h') and
                      hasattr(engine, 'fitSharded') and os.environ.get('SHEPSEG_FIT_SHARDED', '1') != '0')
    if rank == 0:
        npix = args.size * args.size
        value = npix / dt / 1e6
        out = {
            "metric": "Mpixels/sec segmented, %d-band 40k x 40k tiled" % nb,
            "value": round(value, 3), "unit": "Mpixels/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt * 1e3, 2), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "u16", "data": "synthetic",
            "config": {"workload": "%s: tiled %dx%d, %d-band uint16 synthimg v1, tileSize=%d, "
                                   "overlap=%d, k=60, minSegmentSize=50, fixedKMeansInit, tile rows "
                                   "sharded over %d GPUs, image + labels resident in HBM"
                                   % (getattr(args, 'workload', 'c3').upper(), args.size, args.size, nb,
                                      args.tile, args.overlap, world),
                       "tiles": r.numTileRows * r.numTileCols, "workers": args.workers,
                       "max_seg_id": int(r.maxSegId),
                       "stitch": r.stitchMode, "chain_steps_redone": int(r.chainStepsRedone),
                       "tiles_per_rank": tilesPerRank,
                       "transport": getattr(comm, 'transport', type(comm).__name__),
                       "rccl_nranks": rcclRanks,
                       "parallelism": "tiles sharded by area over %d ranks, one process per GPU; the k-means fit %s; "
                                      "overlap strips point to point, histogram all-reduced" % (
                                          world, "with its E-step sharded by sample rows (labels all-gathered per iteration)"
                                          if fitShardedHere else "on rank 0")},
            # (cpu_baseline is a one-GPU figure: `python bench.py --full` prints it; BASELINE.md: the reference's numba
            #  path does ~1.3 Mpixels/s per core)
            "reference_numba_mpx_per_core": 1.3,
            "roofline": {"bound": "hbm", "kernel": "whole path", "achieved": round(
                value * 1e6 * (2 * nb + 4) / 1e9, 3), "peak": 8000.0 * world, "unit": "GB/s",
                "frac": round(value * 1e6 * (2 * nb + 4) / 1e9 / (8000.0 * world), 6),
                "traffic": None},
        }
        print(json.dumps(out), flush=True)
    comm.barrier()
    comm.close()
