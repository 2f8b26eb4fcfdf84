"""The cases of tests/test_gpu_subset_edges.py -- the subset recode of csrc/subset.h at its tile, key-width, id-range
and shard edges -- with a plain model of the recode that shares nothing with the kernels' closed formula.

Importable without a GPU: tests/test_subset_cases_host.py ties the model to the oracle (the reference's visiting loop
in C) and to the reference's goldens before any kernel is compared with it.  Everything is integer work: results are
compared with numpy.array_equal, no tolerance anywhere.

 * visit_keys numbers the window's pixels by walking the tiles (tile rows outer, tile columns inner, raster order
   inside a tile) and counting;
 * model walks the pixels in that order with a dict, as subset.py's processSubsetTile does;
 * shard_first is what a rank holding some window rows must report to the others: per id, the smallest visit key
   among its unmasked pixels in those rows.

The cases (A to E as in test_gpu_subset_edges.py) are Case objects: a label raster, the window, a mask or None, the
tile and the max_seg_id to pass.  The id-range and key-width edges follow the block sizes parsed out of scan.h and
sort.h (prim_cases), so a change of a block size moves the cases with it."""
import numpy as np

from prim_cases import SCAN_SUB, SCAN_ITEMS, SORT_TILE, _seed

LIST_BLOCK = 256            # threads per block of k_subset_first / _list / _lut / _apply / _scatter (subset.h)
HUGE_TILE = 1 << 30         # the tile tilingstats passes for "the whole chunk is one tile"
M32 = 0xFFFFFFFF


# ---- the model -------------------------------------------------------------------------------------------------------
_keys = {}


def visit_keys(ys, xs, T):
    """(ys, xs) int64: each window pixel's position in the visiting order (read-only, computed once per geometry)"""
    have = _keys.get((ys, xs, T))
    if have is not None:
        return have
    keys = np.full((ys, xs), -1, dtype=np.int64)
    k = 0
    for ty in range(0, ys, T):                      # tile rows
        for tx in range(0, xs, T):                  # tile columns
            for y in range(ty, min(ty + T, ys)):    # raster order inside the tile
                for x in range(tx, min(tx + T, xs)):
                    keys[y, x] = k
                    k += 1
    keys.flags.writeable = False
    _keys[(ys, xs, T)] = keys
    return keys


def visit_order(ys, xs, T):
    "the window's pixels (y, x) as two lists, in visiting order"
    order = np.argsort(visit_keys(ys, xs, T), axis=None, kind='stable')
    return (order // max(xs, 1)).tolist(), (order % max(xs, 1)).tolist()


def model(seg, tlx, tly, xs, ys, mask, T):
    """(out (ys, xs) uint32, orig, hist): every unmasked non-null id gets the next new id when first visited;
    orig[new] = old and hist[new] = pixels, row 0 of both is 0"""
    out = np.zeros((ys, xs), dtype=np.uint32)
    new = {}
    orig, hist = [0], [0]
    yy, xx = visit_order(ys, xs, T)
    for y, x in zip(yy, xx):
        s = int(seg[tly + y, tlx + x])
        if s == 0 or (mask is not None and mask[y, x] == 0):
            continue
        v = new.get(s)
        if v is None:
            v = new[s] = len(orig)
            orig.append(s)
            hist.append(0)
        hist[v] += 1
        out[y, x] = v
    return out, np.array(orig, dtype=np.uint32), np.array(hist, dtype=np.uint32)


def shard_first(seg, tlx, tly, xs, ys, mask, T, rows):
    """(keys, ids), ids ascending: per id with an unmasked pixel in window rows [rows[0], rows[1]), the smallest
    visit key among those pixels"""
    keys = visit_keys(ys, xs, T)
    first = {}
    for y in range(rows[0], rows[1]):
        for x in range(xs):
            s = int(seg[tly + y, tlx + x])
            if s == 0 or (mask is not None and mask[y, x] == 0):
                continue
            k = int(keys[y, x])
            if s not in first or k < first[s]:
                first[s] = k
    ids = sorted(first)
    return np.array([first[s] for s in ids], dtype=np.uint32), np.array(ids, dtype=np.uint32)


def merge_first(parts, max_id=M32):
    """orig (row 0 = 0) from the (keys, ids) of any number of shards: ids 1..max_id ordered by their minimum key"""
    first = {}
    for keys, ids in parts:
        for k, s in zip(keys.tolist(), ids.tolist()):
            if s == 0 or s > max_id:
                continue
            if s not in first or k < first[s]:
                first[s] = k
    return np.array([0] + sorted(first, key=lambda s: first[s]), dtype=np.uint32)


def held_rows(lo, hi, tly, ys):
    "the window rows [a, b) that image rows [lo, hi) hold"
    a = min(max(0, lo - tly), ys)
    return a, max(a, min(ys, hi - tly))


# ---- cases -----------------------------------------------------------------------------------------------------------
class Case(object):
    """seg: (rows, cols) uint32 raster; the window (tlx, tly, xs, ys); mask (ys, xs) uint8 or None; T; max_seg_id"""

    def __init__(self, name, seg, win, mask, T, max_seg_id=None):
        self.name, self.mask, self.T = name, mask, T
        self.seg = np.ascontiguousarray(seg, dtype=np.uint32)
        (self.tlx, self.tly, self.xs, self.ys) = win
        self.max_seg_id = int(self.seg.max()) if max_seg_id is None else max_seg_id
        self.seg.flags.writeable = False
        if mask is not None:
            assert mask.shape == (self.ys, self.xs) and mask.dtype == np.uint8
            mask.flags.writeable = False
        self._want = None
        self._base = None

    @property
    def win(self):
        return (self.tlx, self.tly, self.xs, self.ys)

    @property
    def args(self):
        "the arguments of model / oracle.subset_recode after seg"
        return (self.tlx, self.tly, self.xs, self.ys, self.mask, self.T)

    def want(self):
        "model(...) of the case, computed once and read-only"
        if self._base is not None:
            return self._base.want()
        if self._want is None:
            self._want = model(self.seg, *self.args)
            for a in self._want:
                a.flags.writeable = False
        return self._want

    def with_max(self, max_seg_id):
        "the same case under another max_seg_id: the result does not depend on it"
        c = Case('%s-max%d' % (self.name, max_seg_id), self.seg, self.win, self.mask, self.T, max_seg_id)
        c._base = self
        return c


def placed(win_labels, tlx, tly, outside):
    """a raster of (tly + ys, tlx + xs) labels with win_labels at (tlx, tly) -- the window touches the raster's
    bottom-right corner -- and `outside` everywhere else"""
    (ys, xs) = win_labels.shape
    seg = np.empty((tly + ys, tlx + xs), dtype=np.uint32)
    seg[:] = outside
    seg[tly:, tlx:] = win_labels
    return seg


# A: every pixel's key.  (ys, xs, T)
GEOMETRIES = ((1, 1, 1), (1, 1, 7), (5, 7, 1), (7, 5, 2), (8, 8, 4), (9, 10, 3), (9, 10, 4), (13, 6, 5), (6, 13, 5),
              (10, 10, 16), (10, 10, HUGE_TILE), (3, 40, 16), (40, 3, 16))
PLACE = (3, 2)              # tlx, tly of the placed runs


def perm_case(ys, xs, T, place):
    """labels a permutation of 1..n in raster order: out must be visit_keys + 1, hist all ones.  Placed: the rows
    above and the columns left of the window hold ids of the window shifted by one pixel, so a wrong offset or
    pitch renumbers"""
    n = ys * xs
    win = np.arange(1, n + 1, dtype=np.uint32).reshape(ys, xs)
    name = 'perm-%dx%d-T%d' % (ys, xs, T)
    if not place:
        return Case(name, win, (0, 0, xs, ys), None, T)
    (tlx, tly) = PLACE
    seg = placed(win, tlx, tly, 0)
    big = np.arange(seg.size, dtype=np.uint32).reshape(seg.shape) % np.uint32(n) + np.uint32(1)
    seg[:tly, :] = big[:tly, :]
    seg[:, :tlx] = big[:, :tlx]
    return Case(name + '-placed', seg, (tlx, tly, xs, ys), None, T)


PERM_CASES = [perm_case(ys, xs, T, place) for (ys, xs, T) in GEOMETRIES for place in (False, True)]


def blocky_labels(by, bx, bh, bw, seed, nids=None):
    """by x bx blocks of bh x bw pixels, ids scrambled (nids given: drawn from 1..nids, so an id comes back in
    blocks far apart)"""
    rng = np.random.RandomState(_seed(seed))
    if nids is None:
        base = rng.permutation(np.arange(1, by * bx + 1)).reshape(by, bx)
    else:
        base = rng.randint(1, nids + 1, size=(by, bx))
    return np.kron(base.astype(np.uint32), np.ones((bh, bw), dtype=np.uint32))


def first_pixels(seg, tlx, tly, xs, ys, mask, T):
    "per id, the (y, x) of its first unmasked pixel in visiting order"
    seen = {}
    yy, xx = visit_order(ys, xs, T)
    for y, x in zip(yy, xx):
        s = int(seg[tly + y, tlx + x])
        if s and s not in seen and (mask is None or mask[y, x]):
            seen[s] = (y, x)
    return seen


BLOCKY_TILES = (3, 8, 64)
BLOCKY_MASKS = ('nomask', 'hide-first', 'hide-ids')


def blocky_case(T, masking):
    """blocks of 5 x 7 (runs shorter than a tile of 8 and 64, longer than one of 3), a ragged window off the block
    grid.  hide-first: the mask hides every id's first-seen pixel, so each first moves to the id's second pixel;
    hide-ids: it hides every pixel of every third id, so the numbering closes up"""
    seg = blocky_labels(6, 5, 5, 7, 'blocky')               # 30 x 35
    seg.ravel()[::41] = 0
    win = (2, 1, 31, 27)
    (tlx, tly, xs, ys) = win
    mask = None
    if masking == 'hide-first':
        mask = np.ones((ys, xs), dtype=np.uint8)
        for (y, x) in first_pixels(seg, tlx, tly, xs, ys, None, T).values():
            mask[y, x] = 0
    elif masking == 'hide-ids':
        mask = (seg[tly:tly + ys, tlx:tlx + xs] % 3 != 0).astype(np.uint8)
    else:
        assert masking == 'nomask'
    return Case('blocky-T%d-%s' % (T, masking), seg, win, mask, T)


BLOCKY_CASES = [blocky_case(T, m) for T in BLOCKY_TILES for m in BLOCKY_MASKS]

# B: key width.  Windows of 2^8 - 1, 2^8, 2^8 + 1, 2^16 - 1, 2^16 and 2^16 + 1 pixels: (ys, xs)
WIDTH_WINDOWS = ((1, 255), (16, 16), (1, 257), (257, 1), (255, 257), (256, 256), (1, 65537), (65537, 1))
WIDTH_TILES = (1024, HUGE_TILE)
WIDTH_FILLS = ('distinct', 'last-pixel')


def width_case(ys, xs, T, fill):
    """distinct: every pixel an id of its own, scrambled -- m = n ids, beyond SORT_TILE and SCAN_ITEMS at the larger
    windows, every key present.  last-pixel: three large segments whose ids fall as their first keys rise, and id 1
    on the last pixel visited alone -- its key n - 1 is the only one with the top bit of the key width set, and a
    sort that drops that bit leaves it where the id order put it: first"""
    n = ys * xs
    name = 'width-%dx%d-T%d-%s' % (ys, xs, T, fill)
    if fill == 'distinct':
        rng = np.random.RandomState(_seed('width-%d' % n))
        return Case(name, (rng.permutation(n) + 1).reshape(ys, xs), (0, 0, xs, ys), None, T)
    assert fill == 'last-pixel'
    keys = visit_keys(ys, xs, T)
    win = np.empty((ys, xs), dtype=np.uint32)
    win[keys < n // 3] = 900
    win[(keys >= n // 3) & (keys < n - n // 4)] = 500
    win[keys >= n - n // 4] = 40
    win[keys == n - 1] = 1
    return Case(name, win, (0, 0, xs, ys), None, T)


WIDTH_CASES = [width_case(ys, xs, T, fill) for (ys, xs) in WIDTH_WINDOWS for T in WIDTH_TILES for fill in WIDTH_FILLS]

# C: id range.  The ids present sit on both sides of the scan's sub-block and block edges and of the 256-thread grid
RANGE_IDS = (1, 255, 256, 257, SCAN_SUB, SCAN_SUB + 1, SCAN_ITEMS, SCAN_ITEMS + 1)
RANGE_WIN = (3, 2, 16, 16)
RANGE_T = 5


def range_seg():
    """a 20 x 21 raster whose 16 x 16 window at (3, 2) holds RANGE_IDS, a few ids between them and nulls, in an
    order that is not the id order; the pixels outside the window hold other ids"""
    rng = np.random.RandomState(_seed('range'))
    ids = np.array(sorted(set(RANGE_IDS + (2, 300, SCAN_SUB // 2, SCAN_ITEMS - 1, 0))), dtype=np.uint32)
    win = ids[rng.randint(0, ids.size, size=(16, 16))]
    win.ravel()[rng.permutation(256)[:len(RANGE_IDS)]] = RANGE_IDS          # each is there at least once
    seg = placed(win, RANGE_WIN[0], RANGE_WIN[1], 0)
    out = rng.randint(1, SCAN_ITEMS + 2, size=seg.shape).astype(np.uint32)
    seg[:RANGE_WIN[1], :] = out[:RANGE_WIN[1], :]
    seg[:, :RANGE_WIN[0]] = out[:, :RANGE_WIN[0]]
    return seg


def range_max_ids(true_max):
    "max_seg_id values: the true maximum, around the next multiple of the 256-thread block, and far above"
    mult = (true_max // LIST_BLOCK + 1) * LIST_BLOCK
    return (true_max, mult - 1, mult, mult + 1, 1 << 20)


def _range_cases():
    mask = np.ones((16, 16), dtype=np.uint8)
    mask[::3, 1::2] = 0
    seg = range_seg()
    true_max = int(seg[2:, 3:].max())
    assert true_max == SCAN_ITEMS + 1
    out = []
    for (tag, m) in (('nomask', None), ('mask', mask)):
        base = Case('range-%s' % tag, seg, RANGE_WIN, m, RANGE_T, true_max)
        out += [base.with_max(v) for v in range_max_ids(true_max)]
    return out


RANGE_CASES = _range_cases()


def _single_id_cases():
    """m = 1: only id 1 present under every max_seg_id, and only id max_seg_id present -- also where max_seg_id + 1,
    the number of ids scanned, ends a sub-block or a block of the scan or begins the next"""
    out = []
    hole = np.ones((16, 16), dtype=np.uint32)
    hole[0, 0] = hole[7, 9] = 0
    for v in (1, SCAN_SUB - 1, SCAN_SUB, SCAN_ITEMS - 1, SCAN_ITEMS) + range_max_ids(SCAN_ITEMS + 1):
        out.append(Case('only-1-max%d' % v, placed(hole, 3, 2, 1), RANGE_WIN, None, RANGE_T, v))
        out.append(Case('only-max-max%d' % v, placed(hole * np.uint32(v), 3, 2, 1), RANGE_WIN, None, RANGE_T, v))
    return out


SINGLE_ID_CASES = _single_id_cases()

# E: shards.  A 47 x 35 raster, the window 30 wide and 40 high from image row 3: rows above and below it are left
SHARD_ROWS, SHARD_COLS = 47, 35
SHARD_WIN = (2, 3, 30, 40)
SHARD_MAX_ID = 300          # the ids are 1..24: more than one 256-thread block is scanned and listed
SHARD_TILES = (8, 7)
SHARD_LAYOUTS = ('on-tile-row', 'row-above', 'row-below', 'single-rows', 'above-and-below', 'one-shard')


def shard_case(T, masked):
    """ids drawn from 1..24 for blocks of 7 x 5, so an id comes back rows apart and its first pixel may lie in any
    shard; a block column begins with the window's ragged last tile column at tile 7 and inside it at tile 8, and
    block rows straddle the tile rows; nulls; the mask hides a pattern that is no multiple of the tile"""
    seg = blocky_labels(7, 7, 7, 5, 'shards', nids=24)[:SHARD_ROWS, :SHARD_COLS].copy()
    seg.ravel()[::29] = 0
    mask = None
    if masked:
        (ys, xs) = (SHARD_WIN[3], SHARD_WIN[2])
        mask = ((np.arange(ys)[:, None] * 5 + np.arange(xs)[None, :] * 3) % 11 > 2).astype(np.uint8)
    return Case('shards-T%d-%s' % (T, 'mask' if masked else 'nomask'), seg, SHARD_WIN, mask, T, SHARD_MAX_ID)


SHARD_CASES = {(T, masked): shard_case(T, masked) for T in SHARD_TILES for masked in (False, True)}


def shard_cuts(layout, T):
    """image-row boundaries 0 = c0 <= c1 <= ... = SHARD_ROWS of a layout; shard r holds image rows [c_r, c_r+1)"""
    tly, ys = SHARD_WIN[1], SHARD_WIN[3]
    edge = tly + 2 * T                          # image row of the window's third tile row
    if layout == 'on-tile-row':
        return [0, edge, SHARD_ROWS]
    if layout == 'row-above':
        return [0, edge - 1, SHARD_ROWS]
    if layout == 'row-below':
        return [0, edge + 1, SHARD_ROWS]
    if layout == 'single-rows':
        return list(range(SHARD_ROWS + 1))
    if layout == 'above-and-below':             # the first shard ends where the window begins, the last begins where it ends
        return [0, tly, edge, tly + ys, SHARD_ROWS]
    assert layout == 'one-shard'
    return [0, SHARD_ROWS]


# hand-built gathered pairs: only the numbering of shp_dsubset_merge_dev is looked at
PAIRS_MAX_ID = 20
PAIRS_SLOT = 6
PAIRS_WIN = (40, 30)        # xs, ys: keys below 1200 take two sort passes
PAIRS_PAD = 2               # what the slot padding holds: read as a pair it says "id 2 at key 2"
PAIRS_RANKS = (
    # rank 0: keys not sorted; id 7 at 30
    ([50, 1000, 10, 30], [5, 3, 9, 7]),
    # rank 1: id 0 and ids above max_seg_id at the smallest keys -- dropped; id 7 at 25
    ([0, 1, 25, 2, 700], [0, PAIRS_MAX_ID + 1, 7, M32, 2]),
    # rank 2: nothing
    ([], []),
    # rank 3: id 7 at 4, its minimum, on the last rank; id 20 = max_seg_id; id 5 again, later than on rank 0
    ([300, 4, 60], [20, 7, 5]),
)
PAIRS_ORIG = (0, 7, 9, 5, 20, 2, 3)         # by minimum key: 4, 10, 50, 300, 700, 1000


def gathered_pairs():
    "(words of the gathered buffer, counts): per rank a slot of 2 * PAIRS_SLOT words -- keys, ids, then padding"
    words = np.full(len(PAIRS_RANKS) * 2 * PAIRS_SLOT, PAIRS_PAD, dtype=np.uint32)
    counts = []
    for r, (keys, ids) in enumerate(PAIRS_RANKS):
        n = len(keys)
        assert n == len(ids) and n < PAIRS_SLOT
        words[r * 2 * PAIRS_SLOT:][:2 * n] = keys + ids
        counts.append(n)
    return words, np.array(counts, dtype=np.uint32)


ALL_CASES = PERM_CASES + BLOCKY_CASES + WIDTH_CASES + RANGE_CASES + SINGLE_ID_CASES + list(SHARD_CASES.values())
assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)
assert SORT_TILE < 65535 and SCAN_ITEMS < 65535, 'the distinct fillings no longer cross the sort and scan blocks'
