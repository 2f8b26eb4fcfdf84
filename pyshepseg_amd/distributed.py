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
  localStatsBands, gatherFlaggedBands, statsOfPairsBands (optional statsBandsOnDevice), or localStats,
      gatherFlagged, statsOfPairs: calcPerSegmentStatsDistributed[Bands] (the protocol: _distributedStats).
  spatialOnDevice (optional): calcPerSegmentSpatialStatsDistributed.
  subsetOnDevice (optional): subsetImageDistributed.
  outputRows(y0, y1) -> image rows [y0, y1) of the kept output (inside outRows), uint32, on the host;
      overviewRects(table, npacked) -> the pixels of a table of overview rectangles (overviewTable), packed:
      writeOutputDistributed, after finish.
  colourTableOnDevice, renderOnDevice (optional): writeColorTableFromRatColumnsDistributed,
      renderColourTableDistributed.
  neighboursOnDevice (optional): findSegmentNeighboursDistributed; reduceOverNeighboursDistributed needs only
      the engine's context ``c``.
"""
import collections
import collections.abc
import contextlib
import ctypes
import sys
import json
import os
import time

import numpy

from . import _lib
from . import shepseg
from . import tiling


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


def idRange(rank, world, maxSegId):
    """This rank's share [lo, hi) of the id space 0..maxSegId for the reduction of straddling segments
    ('GPU g owns ids in [g S / N, (g + 1) S / N)')."""
    ns = int(maxSegId) + 1
    return (rank * ns) // world, ((rank + 1) * ns) // world


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
    from . import comm as _comm
    from . import tilingstats
    if not hasattr(engine, 'spatialOnDevice'):
        raise tilingstats.PyShepSegStatsError("the distributed spatial statistics need a device engine (HipEngine)")
    dcomm = comm if getattr(comm, 'onDevice', False) else _comm.HostStagedDev(comm, engine.c)
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
    if isinstance(hist, tuple):
        (d_hist, ns, ownHist) = (ctypes.c_void_p(hist[1]), int(hist[2]), False)
    else:
        h32 = numpy.ascontiguousarray(hist, dtype=numpy.uint32)
        ns = len(h32)
        d_hist = tiling._devAlloc(c, ns * 4)
        c.check(L.shp_dev_upload(c.handle, d_hist, _lib.ptr(h32), ns * 4))
        ownHist = True
    S = ns - 1
    colWords = ((nInt * 8 + nFloat * 4) * ns + 7) // 8
    # (blocks from / back to the driver's cache of device scratch blocks: a 1.2-GB hipMalloc per call otherwise)
    d_cols = tiling._devAlloc(c, colWords * 8)
    toFree = [(d_cols, colWords * 8)] + ([(d_hist, ns * 4)] if ownHist else [])
    try:
        c.check(L.shp_dev_memset(c.handle, ctypes.c_void_p(d_cols.value + (colWords - 1) * 8), 0, 8))
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
        slot = max(counts)
        slotRow = (slot * itemsize + 15) // 16 * 16           # a plane's row of a rank's block: the same on every rank
        (merged, nIds) = (ctypes.c_int64(0), ctypes.c_int64(0))
        if slot > 0:
            bufs = []
            for sz in (slot * 4, nPlanes * slotRow, comm.world * slot * 4, comm.world * nPlanes * slotRow):
                p = tiling._devAlloc(c, sz)
                bufs.append(p)
                toFree.append((p, sz))
            (d_sendS, d_sendV, d_allS, d_allV) = bufs
            if nPairs.value:
                c.check(L.shp_dev_copy(c.handle, d_sendS, pSeg, nPairs.value * 4))
                for p in range(nPlanes):
                    c.check(L.shp_dev_copy(c.handle, ctypes.c_void_p(d_sendV.value + p * slotRow),
                                           ctypes.c_void_p(pVal.value + p * rowBytes.value), nPairs.value * itemsize))
            comm.allgather_dev(d_sendS.value, d_allS.value, slot * 4)
            comm.allgather_dev(d_sendV.value, d_allV.value, nPlanes * slotRow)
            (lo, hi) = idRange(comm.rank, comm.world, S)
            cnts = numpy.array(counts, dtype=numpy.uint32)
            c.check(L.shp_dstats_merge_bands_dev(c.handle, d_allS, d_allV, slot, slotRow, comm.world, _lib.ptr(cnts),
                                                 dtypeCode, nBandsIn, nPlanes, _lib.ptr(planeOfBand), S, _lib.ptr(hasNull),
                                                 _lib.ptr(nullVals), _lib.ptr(fast), _lib.ptr(perBand), int(missing), lo, hi,
                                                 d_cols, ctypes.byref(merged), ctypes.byref(nIds)))
        if comm.world > 1:
            comm.allreduce_dev_i64(d_cols.value, colWords)
        (ic, fc) = (None, None)
        if fetch:
            ic = numpy.empty((nInt, ns), dtype=numpy.int64)
            fc = numpy.empty((nFloat, ns), dtype=numpy.float32)
        if fetch and nInt:
            c.check(L.shp_dev_download(c.handle, _lib.ptr(ic), d_cols, ic.nbytes))
        if fetch and nFloat:
            c.check(L.shp_dev_download(c.handle, _lib.ptr(fc), ctypes.c_void_p(d_cols.value + nInt * 8 * ns), fc.nbytes))
    finally:
        for (p, sz) in toFree:
            tiling._devRelease(c, p, sz)
    # the job's figures: the ranks' id shares partition the straddlers, the ranks' rows their pixels
    tot = comm.allgather_obj((int(nIds.value), int(nPairs.value)))
    nPix = int(sum(t[1] for t in tot))
    return ic, fc, int(sum(t[0] for t in tot)), nPix, nPix * (4 + nPlanes * itemsize)


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


_DTYPE_SIZE = {0: 1, 1: 2, 2: 2, 3: 4, 4: 4}


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
    errs = [x[3] for x in ctrl if x[3]]
    if errs:
        raise Err(errs[0])
    if len({x[4] for x in ctrl}) != 1:
        raise Err("the ranks pass different kinds of user function (built-in on some, user-defined on others)")
    ranges = [(x[0], x[1]) for x in ctrl]
    codes = {x[2] for x in ctrl if x[2] >= 0}
    if len(codes) != 1:
        raise Err("the ranks' bands differ in data type (%s)" % sorted(codes))
    dtypeCode = codes.pop()
    isz = _DTYPE_SIZE[dtypeCode]
    if nRows is None:
        nRows = max(b for (a, b) in ranges)
    if isUser:
        return _userFuncSpatialStats(c, comm, d_seg, d_band, dtypeCode, int(nRows), nCols, rowRange, hist, nInt,
                                     nFloat, userFunc, userParam, missing, imgNullVal, fetch, int(tileSize),
                                     batchPoints, info)
    (above, below) = {0: (0, 0), 1: (1, 1), 2: (0, int(params[0]))}[func]
    plan = spatialHaloPlan(ranges, comm.rank, nRows, above, below)     # (raises alike on every rank)
    (lo, hi) = (int(rowRange[0]), int(rowRange[1]))
    h = max(hi - lo, 0)
    (ha, hb) = (plan['above'], plan['below'])
    toFree = []

    def alloc(nbytes):
        p = tiling._devAlloc(c, nbytes)
        toFree.append((p, nbytes))
        return p
    if isinstance(hist, tuple):
        (d_hist, ns) = (ctypes.c_void_p(hist[1]), int(hist[2]))
    else:
        h32 = numpy.ascontiguousarray(hist, dtype=numpy.uint32)
        ns = len(h32)
        d_hist = alloc(ns * 4)
        c.check(L.shp_dev_upload(c.handle, d_hist, _lib.ptr(h32), ns * 4))
    S = ns - 1
    colWords = ((nInt * 8 + nFloat * 4) * ns + 7) // 8
    try:
        d_cols = alloc(colWords * 8)
        c.check(L.shp_dev_memset(c.handle, ctypes.c_void_p(d_cols.value + (colWords - 1) * 8), 0, 8))
        # ---- halo rows: every rank's first / last rows in one all-gather of labels and one of band values
        halo = {'segUp': None, 'bandUp': None, 'segDn': None, 'bandDn': None}
        slot = plan['slot']
        if slot and comm.world > 1:
            rowB = (nCols * 4, nCols * isz)
            sends = [alloc(max(slot * nCols * b, 1)) for b in rowB]
            alls = [alloc(max(comm.world * slot * nCols * b, 1)) for b in rowB]
            for (ownRow, slotRow, n) in plan['send']:
                for (k, src) in enumerate((d_seg, d_band)):
                    c.check(L.shp_dev_copy(c.handle, ctypes.c_void_p(sends[k].value + slotRow * rowB[k]),
                                           ctypes.c_void_p(src + ownRow * rowB[k]), n * rowB[k]))
            for k in range(2):
                comm.allgather_dev(sends[k].value, alls[k].value, slot * rowB[k])
            for (key, rows, recv) in (('Up', ha, plan['recvAbove']), ('Dn', hb, plan['recvBelow'])):
                if not rows:
                    continue
                bufs = [alloc(rows * b) for b in rowB]
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
        over = sum(g[1][0] for g in got)
        (px, hpx) = (sum(g[1][1] for g in got), got[0][1][2])
        if over or px != hpx:
            raise Err("the segment histogram does not match the label raster (%d ids with more pixels on one rank "
                      "than the histogram says; %d labelled pixels, %d in the histogram)" % (over, px, hpx))
        counts = [g[0] for g in got]
        recSlot = max(counts)
        nIds = ctypes.c_int64(0)
        if recSlot > 0:
            nb = recSlot * int(W.value) * 8
            d_send = alloc(nb)
            d_all = alloc(comm.world * nb)
            if nRec.value:
                c.check(L.shp_dev_copy(c.handle, d_send, pRec, nRec.value * int(W.value) * 8))
            comm.allgather_dev(d_send.value, d_all.value, nb)
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
        (ic, fc) = (None, None)
        if fetch:
            ic = numpy.empty((nInt, ns), dtype=numpy.int64)
            fc = numpy.empty((nFloat, ns), dtype=numpy.float32)
        if fetch and nInt:
            c.check(L.shp_dev_download(c.handle, _lib.ptr(ic), d_cols, ic.nbytes))
        if fetch and nFloat:
            c.check(L.shp_dev_download(c.handle, _lib.ptr(fc), ctypes.c_void_p(d_cols.value + nInt * 8 * ns), fc.nbytes))
    finally:
        for (p, sz) in toFree:
            tiling._devRelease(c, p, sz)
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


def subsetHeldRows(rowRange, tly, ys):
    """The window rows [a, b) that output rows rowRange = (outLo, outHi) hold of a window of ys rows from image
    row tly: [max(0, outLo - tly), min(ys, outHi - tly)), as (a, a) when they hold none (host only)."""
    (lo, hi, tly, ys) = (int(rowRange[0]), int(rowRange[1]), int(tly), int(ys))
    a = min(max(0, lo - tly), ys)
    return a, max(a, min(ys, hi - tly))


def disjointRowsError(rowRanges, what):
    """None when the ranks' output rows (outLo, outHi) do not overlap, else the message that refuses them for
    ``what`` (tile-sharded runs share rows)."""
    live = sorted((int(a), int(b)) for (a, b) in rowRanges if b > a)
    for (x, y) in zip(live, live[1:]):
        if x[1] > y[0]:
            return ("%s needs ranks with disjoint output rows (rows %d..%d and %d..%d overlap): run the "
                    "segmentation with SHEPSEG_SHARD=rows" % (what, x[0], x[1], y[0], y[1]))
    return None


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
    if nRows is None:
        nRows = max(b for (a, b) in ranges)
    err = disjointRowsError(ranges, 'subsetImageDistributed')
    maskArr = None
    try:
        if err is None:
            subset.checkWindow(int(nRows), int(nCols), tlx, tly, xs, ys)
            maskArr = subset.loadMask(mask, xs, ys)
            if tileSize < 1:
                err = "tileSize must be positive"
    except Err as e:
        err = str(e)
    errs = [x for x in comm.allgather_obj(err) if x]
    if errs:
        raise Err(errs[0])
    L = c._L
    (lo, hi) = ranges[comm.rank]
    (a, b) = subsetHeldRows((lo, hi), tly, ys)
    h = max(hi - lo, 0)
    toFree = []

    def alloc(nbytes):
        p = tiling._devAlloc(c, max(int(nbytes), 16))
        toFree.append((p, max(int(nbytes), 16)))
        return p
    try:
        d_mask = None
        if maskArr is not None and b > a:
            part = numpy.ascontiguousarray(maskArr[a:b])
            d_mask = alloc(part.nbytes)
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
        slot = max(counts)
        d_send = alloc(slot * 8)
        d_all = alloc(comm.world * slot * 8)
        if nPairs.value:
            c.check(L.shp_dev_copy(c.handle, d_send, pPairs, nPairs.value * 8))
        comm.allgather_dev(d_send.value, d_all.value, slot * 8)
        # hist as uint32 lanes of int64 words: no id has 2^32 pixels in the window, so no carry crosses a lane
        cap = sum(counts) + 1
        cap += cap % 2
        d_hist = alloc(cap * 4)
        d_rows = alloc((b - a) * xs * 4)
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
    finally:
        for (p, sz) in toFree:
            tiling._devRelease(c, p, sz)
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
    from . import comm as _comm
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
    errs = [x for x in comm.allgather_obj(err) if x]
    if errs:
        raise Err(errs[0])
    dcomm = comm if getattr(comm, 'onDevice', False) else _comm.HostStagedDev(comm, engine.c)
    (rows, (a, b), orig, hist) = engine.subsetOnDevice(dcomm, result.maxSegId, tlx, tly, newXsize, newYsize,
                                                       mask=maskImage, tileSize=tileSize)
    res = subset.SubsetResult()
    (res.segimg, res.rows, res.origSegIds, res.hist) = (rows, (a, b), orig, hist)
    res.columns = subset.recodeColumns(orig, hist, ratColumns, origSegIdColName)
    if outname is not None:
        _writeRows(comm, outname, rows, a, (int(newYsize), int(newXsize)))
    return res


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
    toFree = []

    def alloc(nbytes):
        p = tiling._devAlloc(c, nbytes)
        toFree.append((p, nbytes))
        return p
    pc = None
    try:
        if isinstance(hist, tuple):
            (d_hist, ns) = (ctypes.c_void_p(hist[1]), int(hist[2]))
            h32 = numpy.empty(ns, dtype=numpy.uint32)
            c.check(L.shp_dev_download(c.handle, _lib.ptr(h32), d_hist, ns * 4))
        else:
            h32 = numpy.ascontiguousarray(hist, dtype=numpy.uint32)
            ns = len(h32)
            d_hist = alloc(ns * 4)
            c.check(L.shp_dev_upload(c.handle, d_hist, _lib.ptr(h32), ns * 4))
        S = ns - 1
        pc = _lib.Context(device=c.device)
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
        (overAll, px, hpx) = (sum(g[1] for g in got), sum(g[2] for g in got), int(hist64[1:].sum()))
        if overAll or px != hpx:
            raise Err("the segment histogram does not match the label raster (%d ids with more pixels on one rank "
                      "than the histogram says; %d labelled pixels, %d in the histogram)" % (overAll, px, hpx))
        counts = [g[0] for g in got]
        slot = max(counts)
        (idLo, idHi) = idRange(comm.rank, comm.world, S)
        d_all = None
        if slot > 0:
            nb = slot * SEGPOINT_RECORD_BYTES
            d_send = alloc(nb)
            d_all = alloc(comm.world * nb)
            if nRec.value:
                c.check(L.shp_dev_copy(c.handle, d_send, pRec, nRec.value * SEGPOINT_RECORD_BYTES))
            comm.allgather_dev(d_send.value, d_all.value, nb)
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
        msg = userFuncErrorOf(errs)
        if msg is not None:
            raise Err(msg)
        clearUnownedRows(ic, fc, owned)
        # ---- the column block: the ranks' rows add up
        if comm.world > 1:
            colWords = ((nInt * 8 + nFloat * 4) * ns + 7) // 8
            block = numpy.zeros(colWords * 8, dtype=numpy.uint8)
            block[:ic.nbytes] = ic.reshape(-1).view(numpy.uint8)
            block[ic.nbytes:ic.nbytes + fc.nbytes] = fc.reshape(-1).view(numpy.uint8)
            d_cols = alloc(colWords * 8)
            c.check(L.shp_dev_upload(c.handle, d_cols, _lib.ptr(block), block.nbytes))
            comm.allreduce_dev_i64(d_cols.value, colWords)
            c.check(L.shp_dev_download(c.handle, _lib.ptr(block), d_cols, block.nbytes))
            ic = block[:ic.nbytes].view(numpy.int64).reshape(nInt, ns).copy()
            fc = block[ic.nbytes:ic.nbytes + fc.nbytes].view(numpy.float32).reshape(nFloat, ns).copy()
    finally:
        for (p, sz) in toFree:
            tiling._devRelease(c, p, sz)
        if pc is not None:
            pc.close()
    # the job's figures: the ranks' id shares partition the straddlers
    tot = comm.allgather_obj((nStradMine, int(nRec.value)))
    nStrad = int(sum(t[0] for t in tot))
    if info is not None:
        info.update(path='points', straddlers=nStrad, points_exchanged=int(sum(t[1] for t in tot)),
                    calls=int(numpy.count_nonzero(ecnt)))
    if not fetch:
        (ic, fc) = (None, None)
    return ic, fc, nStrad, 0


# ------------------------------------------------------------------------------------------
# HIP engine: this rank's GPU
# ------------------------------------------------------------------------------------------
# ---- the segment-neighbour table and its reductions on the row-sharded output (csrc/dneighbours.h) -------------
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
    errs = [x[2] for x in ctrl if x[2]]
    if errs:
        raise Err(errs[0])
    if len({x[3:] for x in ctrl}) != 1:
        raise Err("the ranks pass different maxSegId, columns or connectivity: %s" % sorted({x[3:] for x in ctrl}))
    (S, nCols) = (int(maxSegId), int(nCols))
    ranges = [(x[0], x[1]) for x in ctrl]
    if nRows is None:
        nRows = max(b for (a, b) in ranges)
    nRows = int(nRows)
    err = disjointRowsError(ranges, 'findSegmentNeighboursDistributed') or _rowsCoverError(ranges, nRows)
    if err:
        raise Err(err)
    plan = spatialHaloPlan(ranges, comm.rank, nRows, 0, 1)
    (lo, hi) = ranges[comm.rank]
    h = max(hi - lo, 0)
    (idLo, idHi) = idRange(comm.rank, comm.world, S)
    L = c._L
    timings = {}
    toFree = []

    def alloc(nbytes):
        p = tiling._devAlloc(c, max(int(nbytes), 16))
        toFree.append((p, max(int(nbytes), 16)))
        return p
    try:
        # ---- the halo row: every rank's first row in one all-gather
        d_halo = None
        rowB = nCols * 4
        haloSenders = 0
        if comm.world > 1 and nCols > 0:
            d_send = alloc(rowB)
            d_rows = alloc(comm.world * rowB)
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
        slot = max(counts)
        d_all = None
        if slot > 0:
            d_send = alloc(slot * 16)
            d_all = alloc(comm.world * slot * 16)
            if cnt[2]:
                c.check(L.shp_dev_copy(c.handle, d_send, pTrav, int(cnt[2]) * 16))
            comm.allgather_dev(d_send.value, d_all.value, slot * 16)
        timings['exchange'] = time.perf_counter() - t1
        # ---- the rows of this rank's id share
        t1 = time.perf_counter()
        ns = S + 1
        d_cols = alloc(2 * ns * 8)
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
    finally:
        for (p, sz) in toFree:
            tiling._devRelease(c, p, sz)
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
    from . import comm as _comm
    from . import neighbours
    if not hasattr(engine, 'neighboursOnDevice'):
        raise neighbours.PyShepSegNeighboursError("the distributed neighbour table needs a device engine (HipEngine)")
    dcomm = comm if getattr(comm, 'onDevice', False) else _comm.HostStagedDev(comm, engine.c)
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
    from . import comm as _comm
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
    dcomm = comm if getattr(comm, 'onDevice', False) else _comm.HostStagedDev(comm, c)
    timings = {'upload': 0.0, 'uploaded': False, 'deviceMs': 0.0}
    _makeShareResident(c, share, timings)
    t1 = time.perf_counter()
    ns = share.maxSegId + 1
    bitsOf = [sorted({bit for (_n, bit, _d) in picked}) for (_col, _ctype, picked) in plan]
    nOut = sum(len(b) for b in bitsOf)
    d_out = tiling._devAlloc(c, nOut * ns * 8)
    try:
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
    finally:
        tiling._devRelease(c, d_out, nOut * ns * 8)
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
    errs = [x[0] for x in ctrl if x[0]]
    if errs:
        raise Err(errs[0])
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
        if nRows is None:
            nRows = max(b for (a, b) in ranges)
        nRows = int(nRows)
        nCols = int(nCols)
        err = disjointRowsError(ranges, 'the distributed merge') or _rowsCoverError(ranges, nRows)
        if err:
            raise Err(err)
        (lo, hi) = ranges[comm.rank]
        h = max(hi - lo, 0)
    timings = {'upload': 0.0, 'uploaded': False}
    ms = {}
    toFree = []
    d_out = None
    nbOut = max(h * nCols * 4, 16)

    def alloc(nbytes):
        p = tiling._devAlloc(c, max(int(nbytes), 16))
        toFree.append((p, max(int(nbytes), 16)))
        return p

    def gatherBlocks(src, count, counts, itemBytes):
        """the ranks' blocks of ``count`` items at ``src`` in one all-gather: (device blocks or None, slot)"""
        slot = max(counts)
        if slot == 0:
            return None, 0
        if comm.world == 1:
            return src, count                   # (the rank's own block, where it lies)
        d_send = alloc(slot * itemBytes)
        d_all = alloc(comm.world * slot * itemBytes)
        if count:
            c.check(L.shp_dev_copy(c.handle, d_send, src, count * itemBytes))
        comm.allgather_dev(d_send.value, d_all.value, slot * itemBytes)
        return d_all, slot
    try:
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
        (d_all, slot) = gatherBlocks(pPairs, nPairs, pairCounts, 8)
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
            d_out = tiling._devAlloc(c, nbOut)
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
        (d_allRec, slotRec) = gatherBlocks(pTrav, int(rc[3]), travCounts, 16)
        d_cols = alloc(2 * (M + 1) * 8)
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
                (res.outDev, d_out) = ((d_out.value, h, nCols, nbOut), None)
    finally:
        for (p, sz) in toFree:
            tiling._devRelease(c, p, sz)
        if d_out is not None:
            tiling._devRelease(c, d_out, nbOut)
    timings['total'] = time.perf_counter() - t0
    res.timings = timings
    if info is not None:
        info.update(figures)
    return res


def _mergeDistributed(engine, comm, share, rule, dres, outfile, info):
    from . import comm as _comm
    from . import neighbours
    Err = neighbours.PyShepSegNeighboursError
    if outfile is not None and not (isinstance(outfile, str) and outfile.endswith('.npy')):
        raise Err("outfile must be None or a .npy path")
    if outfile is not None and dres is None:
        raise Err("outfile needs dres: the rows to recode are the engine's kept output")
    dcomm = comm if getattr(comm, 'onDevice', False) else _comm.HostStagedDev(comm, engine.c)
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
        sizes = [m * 4] + [rowBytes] * len(vals)
        blocks = [tiling._devAlloc(self.c, sz) for sz in sizes]
        try:
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
        finally:
            for (p, sz) in zip(blocks, sizes):
                tiling._devRelease(self.c, p, sz)
        return ic[:nInt], fc[:nFloat]

    def statsBandsOnDevice(self, comm, hist, planes, planeOfEntry, fast, perBand, nullVals, nInt, nFloat, missing):
        """calcPerSegmentStatsDistributed[Bands]' device path for this rank's output rows (deviceStatsBands).
        planes: the distinct band numbers, planeOfEntry[e]: which of them entry e reads."""
        held = self.ras is not None and self.outHi > self.outLo
        if held:
            d_out = self._lastOut.value if hasattr(self._lastOut, 'value') else int(self._lastOut)
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
        held = self.ras is not None and self.outHi > self.outLo
        d_out = (self._lastOut.value if hasattr(self._lastOut, 'value') else int(self._lastOut)) if held else 0
        return deviceSpatialStats(self.c, comm, d_out, self._bandPtr(imgbandnum) if held else 0,
                                  _lib.SHP_DTYPES[self.ras.dtype] if self.ras is not None else -1, None, self.nCols,
                                  (self.outLo, self.outHi), hist, colTypes, userFunc, userParam, missing, imgNullVal,
                                  tileSize=tileSize, batchPoints=batchPoints, info=info)

    def subsetOnDevice(self, comm, maxSegId, tlx, tly, xs, ys, mask=None, tileSize=None):
        """subsetImageDistributed's path for this rank's output rows (deviceSubset)."""
        held = self.outHi > self.outLo
        d_out = (self._lastOut.value if hasattr(self._lastOut, 'value') else int(self._lastOut)) if held else 0
        return deviceSubset(self.c, comm, d_out, None, self.nCols, (self.outLo, self.outHi), maxSegId, tlx, tly, xs,
                            ys, mask=mask, tileSize=tileSize)

    def neighboursOnDevice(self, comm, maxSegId, fourConnected=True, info=None):
        """findSegmentNeighboursDistributed's path for this rank's output rows (deviceNeighbours)."""
        held = self.outHi > self.outLo
        d_out = _addr(self._lastOut) if held else 0
        return deviceNeighbours(self.c, comm, d_out, None, self.nCols, (self.outLo, self.outHi), maxSegId,
                                fourConnected=fourConnected, info=info)

    def mergeOnDevice(self, comm, share, rule, nRows, outfile=None, info=None):
        """mergeSegmentsDistributed's path with this rank's output rows recoded (deviceMerge)."""
        held = self.outHi > self.outLo
        d_out = _addr(self._lastOut) if held else 0
        return deviceMerge(self.c, comm, share, rule, d_out, nRows, self.nCols, (self.outLo, self.outHi), outfile=outfile,
                           info=info)

    def localOutput(self):
        out = numpy.empty((self.outHi - self.outLo, self.nCols), dtype=numpy.uint32)
        self.c.check(self.L.shp_dev_download(self.c.handle, _lib.ptr(out), self._lastOut, out.nbytes))
        return out

    def outputRows(self, y0, y1):
        """image rows [y0, y1) of the kept output (inside outRows), to the host"""
        out = numpy.empty((y1 - y0, self.nCols), dtype=numpy.uint32)
        if out.size:
            d = self._lastOut.value if hasattr(self._lastOut, 'value') else int(self._lastOut)
            self.c.check(self.L.shp_dev_download(self.c.handle, _lib.ptr(out),
                                                 ctypes.c_void_p(d + (y0 - self.outLo) * self.nCols * 4), out.nbytes))
        return out

    def overviewRects(self, table, npacked):
        """the overview rectangles of a writeOutputDistributed table sampled from the kept output in one launch
        (shp_overview_rects_dev), downloaded once: uint32 (npacked,)"""
        out = numpy.empty(npacked, dtype=numpy.uint32)
        if npacked == 0:
            return out
        table = numpy.ascontiguousarray(table, dtype=numpy.int64)
        d = tiling._devAlloc(self.c, npacked * 4)
        try:
            self.c.check(self.L.shp_overview_rects_dev(self.c.handle, self._lastOut,
                                                       (self.outHi - self.outLo) * self.nCols, _lib.ptr(table),
                                                       table.shape[0], d, npacked))
            self.c.check(self.L.shp_dev_download(self.c.handle, _lib.ptr(out), d, out.nbytes))
        finally:
            tiling._devRelease(self.c, d, npacked * 4)
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
        d_out = _addr(self._lastOut) if held else 0
        (d_table, n) = (None, 0)
        try:
            if cols is not None:
                n = len(cols[0])
                d_table = tiling._devAlloc(self.c, n * 4)
                self.c.check(self.L.shp_colour_pack(self.c.handle, _lib.ptr(cols[0]), _lib.ptr(cols[1]),
                                                    _lib.ptr(cols[2]), _lib.ptr(cols[3]), n, d_table))
                table = (d_table, n)
            else:
                table = self.colourTable
            return deviceRender(self.c, comm, d_out, (self.outHi - self.outLo) if held else 0, self.nCols, table[0],
                                table[1], rects=rects, npacked=npacked, sink=sink, blockPixels=blockPixels, info=info)
        finally:
            if d_table is not None:
                tiling._devRelease(self.c, d_table, n * 4)

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
# colour tables and the RGBA rendering on the row-sharded output
# ------------------------------------------------------------------------------------------
RENDER_BLOCK_PIXELS = 1 << 24      # pixels per lookup / download block: 64 MB each way, several blocks per rank
RENDER_GROUP_BLOCKS = 4            # blocks per pinned staging buffer (and per write into the file)
_SEL_PASSES = 8                    # csrc/colour.h: SEL_PASSES, SEL_HIST_WORDS
_SEL_HIST_WORDS = 512
_COL_BAD = {1: "column holds a NaN or an infinity",
            2: "integer column holds a magnitude of 2^53 or more: not exact in float64"}


def _addr(p):
    """a device address as an int (None, an int or a ctypes.c_void_p)"""
    if p is None:
        return 0
    return int(p.value or 0) if hasattr(p, 'value') else int(p)


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
    errs = [g[0] for g in got if g[0]]
    if errs:
        raise Err(errs[0])
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
    toFree = []

    def alloc(nbytes):
        p = tiling._devAlloc(c, nbytes)
        toFree.append((p, nbytes))
        return p
    d_table = tiling._devAlloc(c, n * 4)
    ok = False
    stretch = []
    deviceMs = 0.0
    try:
        d_bytes = alloc(4 * pitch)
        d_send = alloc(slot) if comm.world > 1 else None
        d_all = alloc(comm.world * slot) if comm.world > 1 else None
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
        ok = True
    finally:
        for (p, sz) in toFree:
            tiling._devRelease(c, p, sz)
        if not ok:
            tiling._devRelease(c, d_table, n * 4)
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
    from . import comm as _comm
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
    errs = [x for x in comm.allgather_obj(err) if x]
    if errs:
        raise Err(errs[0])
    dcomm = comm if getattr(comm, 'onDevice', False) else _comm.HostStagedDev(comm, engine.c)
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
    errs = [x for x in comm.allgather_obj(err) if x]
    if errs:
        raise Err(errs[0])
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
    dcomm = comm if getattr(comm, 'onDevice', False) else _comm.HostStagedDev(comm, c)
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
            # (cpu_baseline is a one-GPU figure: `python bench.py` prints it; BASELINE.md: the reference's numba
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
