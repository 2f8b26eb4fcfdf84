"""Label tilings built to reach every rule of the cross-tile stitch, and a plain numpy model of it.

The stitch (pyshepseg_amd/csrc/stitch.h) decides what happens where neighbouring tiles DISAGREE
in their overlap.  Tiles cut from a real segmentation agree almost everywhere, so these cases are
generated instead: every tile is an arbitrary uint32 labelling (ids 1..max without gaps, 0 = null)
of the tiling that oracle.get_tiles gives for (nr, nc, tile, overlap).

model_stitch(case) restates the reference's stitchTiles / recodeTile / recodeSharedSegments /
crossesMidline / relabelSegments (tiling.py:950-1306) with numpy.nonzero, a sort by label and
numpy.unique, and keeps a census of the events a case is there to produce.  The conditions on
that census are asserted by tests/test_stitch_cases_host.py; the device is
compared with the model by tests/test_gpu_stitch_cases.py.

Census of the cases as generated (sums over a group's tilings; `ties` = modes decided by a tie,
`0 wins` = of those won by id 0, `3-way` = three or more values tied, `hi / lo` = the winning id
hashes to the higher / lower slot of the device's pair table than the best loser, `ovr` = the
left strip's mode replaces a different mode of the top strip, `out` = segments that get a new id
without a pixel in the trimmed window, `K!=R` = tiles whose largest new id is not in the window):

    group          tilings  modes  ties  0 wins  3-way   hi / lo   ovr   out  K!=R max id  cross px
    ties                 2    201    38      12      6   11 / 27     3     0     0    578       372
    midline              6    223    38       4      1   19 / 19     1     0     0    220       211
    both_strips          1    306    87       9     28   42 / 45    16     0     0    311       880
    shapes               1     88    13       3      2     5 / 8     1     0     0    359       577
    lane_edges           2     79     9       9      0     5 / 4     0     0     0    131      1464
    outside_owner        1     49     2       1      0     2 / 0     2     4     1    142       772
    dense_pairs          1     14    14       0     14     8 / 6     0     0     0   3120       992
    many_segments        1    296     0       0      0     0 / 0     0     0     0   9409       384
    grids                3    192    10       2      0     4 / 6     6     1     1     81       468
    random              20   1319    91      25      7   46 / 45    32     2     2    334       535
"""
import numpy as np

from oracle import oracle as orc

BIG = 0x7FFFFFFF


# ----------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------
class Case(object):
    """One tiling: nr x nc raster, tile size, overlap, and a local labelling per (col, row) tile."""

    def __init__(self, group, name, nr, nc, tile, overlap, make, seed, four=True):
        (self.group, self.name, self.nr, self.nc, self.tile, self.overlap) = (group, name, nr, nc, tile, overlap)
        self.four = four
        self.seed = seed
        self.geom, self.ntc, self.ntr = orc.get_tiles(nr, nc, tile, overlap)
        rng = np.random.default_rng(seed)
        self.tiles = {}
        self._model = {}
        for (col, row) in self.order():
            (_x, _y, xs, ys) = self.geom[(col, row)]
            # make: a callable that labels the tile, or a dict of ready local tiles
            t = np.asarray(make[(col, row)], dtype=np.uint32) if isinstance(make, dict) else \
                compact(make(self, col, row, ys, xs, rng))
            assert t.shape == (ys, xs) and t.dtype == np.uint32
            self.tiles[(col, row)] = t

    def window(self, col, row):
        """(top, bottom, left, right, xout, yout): the trimmed window, tiling.py:997-1022"""
        (xpos, ypos, xs, ys) = self.geom[(col, row)]
        m = int(self.overlap / 2)
        (top, bottom, left, right, xout, yout) = (m, ys - m, m, xs - m, xpos + m, ypos + m)
        if row == 0:
            (top, yout) = (0, ypos)
        if row == self.ntr - 1:
            bottom = ys
        if col == 0:
            (left, xout) = (0, xpos)
        if col == self.ntc - 1:
            right = xs
        return (top, bottom, left, right, xout, yout)

    def order(self):
        return sorted(self.geom, key=lambda k: (k[1], k[0]))          # tiling.py:978

    def __repr__(self):
        return 'Case(%s)' % self.name


def compact(t):
    """ids 1..max without gaps, in the order of the old ids; 0 stays 0"""
    u, inv = np.unique(t, return_inverse=True)
    inv = inv.reshape(t.shape)
    return (inv if u[0] == 0 else inv + 1).astype(np.uint32)


def blocks(rng, ys, xs, bh, bw, jitter=True, nulls=0.0, py=None, px=None):
    """bh x bw blocks of random phase; jitter moves every row / column of pixels by -1, 0 or 1"""
    py = int(rng.integers(0, bh)) if py is None else py
    px = int(rng.integers(0, bw)) if px is None else px
    r = np.arange(ys)[:, None]
    c = np.arange(xs)[None, :]
    jr = rng.integers(-1, 2, size=xs)[None, :] if jitter else 0
    jc = rng.integers(-1, 2, size=ys)[:, None] if jitter else 0
    lab = ((r + py + jr + 1) // bh) * (xs // bw + 4) + (c + px + jc + 1) // bw + 1
    lab = lab.astype(np.int64)
    if nulls:
        lab[rng.random((ys, xs)) < nulls] = 0
    return lab


def _ties(case, col, row, ys, xs, rng):
    # unjittered small blocks: a segment then often covers equally many pixels of two or three of the
    # neighbour's ids, and the neighbour's strip is 0 beyond its own window (ids it does not own)
    (bh, bw) = [(2, 2), (2, 4), (4, 2), (4, 4), (2, 6), (4, 6), (2, 3), (4, 3)][int(rng.integers(0, 8))]
    lab = blocks(rng, ys, xs, bh, bw, jitter=False)
    for _ in range(3):                                  # null rectangles
        (r0, c0) = (int(rng.integers(0, ys - 4)), int(rng.integers(0, xs - 4)))
        lab[r0:r0 + int(rng.integers(1, 5)), c0:c0 + int(rng.integers(1, 9))] = 0
    return lab


def _bands(ys, xs, rbreaks, cbreaks_by_band):
    """label = (row band, column band); the column breaks may differ from row band to row band"""
    rb = np.searchsorted(np.asarray(sorted(set(rbreaks))), np.arange(ys), side='right')
    lab = np.zeros((ys, xs), dtype=np.int64)
    for b in np.unique(rb):
        cb = np.searchsorted(np.asarray(sorted(set(cbreaks_by_band[b % len(cbreaks_by_band)]))), np.arange(xs),
                             side='right')
        lab[rb == b, :] = (b * (xs + 1) + cb + 1)[None, :]
    return lab


def _midline(case, col, row, ys, xs, rng):
    """In the top strip, runs of columns whose segments end at mid - 1, span mid - 1 .. mid, or start at
    mid; the same, transposed, in the left strip below it."""
    o = case.overlap
    mid = o // 2
    w = 2 + (col + 2 * row) % 3                         # run width: differs between neighbours
    lab = np.zeros((ys, xs), dtype=np.int64)
    nxt = 1

    def stripes(n_along, horizontal):
        nonlocal nxt
        out = np.zeros((o + 3, n_along), dtype=np.int64)
        for (k, a) in enumerate(range(0, n_along, w)):
            kind = k % 3
            if kind == 0:
                brk = [mid]                             # [0, mid) ends at mid - 1 | [mid, ..) starts at mid
            elif kind == 1:
                brk = [mid - 1, mid + 1]                # [mid - 1, mid] spans the midline
            else:
                brk = [mid + 1] if mid >= 1 else [1]    # [0, mid] crosses from the strip's first line on
            brk = [b for b in brk if 0 < b < o + 3] + [o + 1]
            band = np.searchsorted(np.asarray(sorted(set(brk))), np.arange(o + 3), side='right')
            out[:, a:a + w] = (nxt + band)[:, None]
            nxt += int(band.max()) + 1
        return out
    body = blocks(rng, ys, xs, 5, 7, jitter=True)
    lab[:, :] = body + 100000
    lab[:o + 3, :] = stripes(xs, True)
    lab[o + 3:, :o + 3] = stripes(ys - o - 3, False).T
    return lab


def _both(case, col, row, ys, xs, rng):
    """Diagonal bands cut by a coarse grid: in the corner where the two strips meet a band crosses both
    midlines, elsewhere one or none; thickness and direction differ between neighbouring tiles."""
    r = np.arange(ys)[:, None]
    c = np.arange(xs)[None, :]
    t = 2 + (col + row) % 2
    d = (r - c) if (col + 2 * row) % 3 else (r - 2 * c)
    band = (d + 4 * (ys + xs) + int(rng.integers(0, t))) // t
    cut = (r // 23) * 64 + (c // 19)
    return band.astype(np.int64) * 4096 + cut + 1


_STAMPS = {
    'U': ['#...#', '#...#', '#...#', '#####'],
    'ring': ['#####', '#...#', '#...#', '#####'],
    'stair8': ['#....', '.#...', '..##.', '....#', '....#'],
    'comb': ['#.#.#.#', '#.#.#.#', '#######'],
    'diag': ['#.....', '.#....', '..#...', '...#..', '....#.', '.....#'],
    'pieces': ['##....', '##....', '......', '......', '....##', '....##'],
}


def stamp_mask(kind, rot):
    m = np.array([[ch == '#' for ch in line] for line in _STAMPS[kind]])
    return np.rot90(m, rot)


def _shapes(case, col, row, ys, xs, rng):
    """Shapes whose extreme pixels are not where a blob has them, across both midlines and across every
    edge of the trimmed window."""
    lab = blocks(rng, ys, xs, 6, 5, jitter=True)
    (top, bottom, left, right, _x, _y) = case.window(col, row)
    o = case.overlap
    mid = o // 2
    nxt = int(lab.max()) + 1
    kinds = sorted(_STAMPS)
    # centres: along the two midlines (which are the window's top and left edges as well) and along the
    # window's bottom and right edges; every line goes through the kinds and their rotations on its own
    count = case.__dict__.setdefault('stamp_count', [0, 3, 1, 4])
    places = []
    for cc in range(10, xs - 8, 9):
        places += [(0, mid, cc), (1, bottom, cc)]
    for rc in range(o + 6, ys - 8, 9):
        places += [(2, rc, mid), (3, rc, right)]
    taken = np.zeros((ys, xs), dtype=bool)
    case.stamped = getattr(case, 'stamped', {})
    for (line, rc, cc) in places:
        n = count[line]
        kind = kinds[n % len(kinds)]
        m = stamp_mask(kind, (n // len(kinds) + line) % 4)
        (h, w) = m.shape
        (r0, c0) = (rc - h // 2, cc - w // 2)
        if (line == 0 and row == 0) or (line == 2 and col == 0):
            continue                                    # no strip here
        count[line] += 1
        if r0 < 0 or c0 < 0 or r0 + h > ys or c0 + w > xs or taken[r0:r0 + h, c0:c0 + w].any():
            continue                                    # off the tile, or it would cut an earlier shape
        lab[r0:r0 + h, c0:c0 + w][m] = nxt
        taken[r0:r0 + h, c0:c0 + w] = True
        case.stamped.setdefault((col, row), []).append((kind, r0, c0, m))
        nxt += 1
    return lab


def _lane_edges(case, col, row, ys, xs, rng):
    """Segments that begin or end exactly at columns 63 / 64 and 127 / 128 and at rows 7 / 8 and 31 / 32
    (the lanes and rows at which a wavefront's or a patch's neighbour pixel comes from elsewhere), and bars
    over the whole strip width, whose pair runs continue from one strip row's end into the next row."""
    o = case.overlap
    mid = o // 2
    rbreaks = [3, 7, mid + 1, mid + 3, o, 31, 32, 40, 63, 64, 66, 95, 96, 127, 128, ys - o, ys - mid, ys - 3]
    if (col + row) % 2:
        rbreaks = [2, 8 if mid > 8 else 0, mid - 2, mid + 2, o + 1, 32, 33, 47, 64, 65, 80, 96, 97, 128, 129,
                   ys - o + 1, ys - mid - 1]
    if col == 0:
        rbreaks = rbreaks + [mid - 1]                   # (and bands that stop short of the midline)
    ca = [mid - 2, mid + 1, 20, 60, 63, 64, 66, 100, 127, 128, xs - o, xs - mid, xs - 2]
    cb = [mid - 1, mid + 1, 24, 57, 64, 65, 90, 128, 129, xs - o + 2, xs - mid + 1]
    cc = [mid, 63, 127, xs - mid]
    full = [xs + 1]                                     # one bar over the whole width
    lab = _bands(ys, xs, [b for b in rbreaks if 0 < b < ys],
                 [[b for b in q if 0 < b < xs] or full for q in (ca, full, cb, cc, full)])
    return lab


def _outside_owner(case, col, row, ys, xs, rng):
    """L-shapes round the trimmed window's bottom-right corner: the bounding box's corner is inside the window,
    no pixel is; they carry the tile's largest local ids."""
    lab = blocks(rng, ys, xs, 7, 6, jitter=True)
    (top, bottom, left, right, _x, _y) = case.window(col, row)
    nxt = int(lab.max()) + 1
    if bottom < ys and right < xs:
        for k in range(min(ys - bottom, xs - right) // 2):
            (r0, c0) = (bottom - 3 - 2 * k, right - 3 - 2 * k)       # the corner of the bounding box
            (rr, cc) = (bottom + 2 * k, right + 2 * k)
            lab[rr, c0:cc + 1] = nxt                    # the horizontal arm, below the window
            lab[r0:rr + 1, cc] = nxt                    # the vertical arm, right of it
            nxt += 1
    return lab


def _dense_pairs(case, col, row, ys, xs, rng):
    """Tile (1, 1): stripes over each strip that cross its midline (nothing in the corner, nothing in the
    margin's part of the other strip).  Its neighbours: one id per pixel of the strip they hand on; an id beyond
    the neighbour's own window also holds the pixel `overlap` lines further in, so that the neighbour owns it."""
    o = case.overlap
    r = np.arange(ys)[:, None]
    c = np.arange(xs)[None, :]
    if (col, row) == (1, 1):
        lab = (blocks(rng, ys, xs, 5, 5, jitter=True) + 1000).astype(np.int64)
        lab[:o, :] = 1 + (c // 11)                      # top strip: stripes 11 columns wide, all o rows
        lab[:, :o] = 500 + (r // 9)
        lab[:o, :o] = 0
        return lab
    lab = (r * xs + c + 1).astype(np.int64)             # an id per pixel
    if row == 0:                                        # hands on its bottom strip: rows ys - o ..
        lab[ys - 2 * o:ys - o, :] = lab[ys - o:, :]
    if col == 0 and row == 1:                           # hands on its right strip
        lab[:, xs - 2 * o:xs - o] = lab[:, xs - o:]
    return lab


def _many(case, col, row, ys, xs, rng):
    # 2 x 2 blocks from (1, 1) on: blocks cover lines 7 .. 8, the midline of an overlap of 16
    return blocks(rng, ys, xs, 2, 2, jitter=False, py=0, px=0)


def _jitter(bh, bw, nulls=0.0):
    def make(case, col, row, ys, xs, rng):
        return blocks(rng, ys, xs, bh + int(rng.integers(0, 3)), bw + int(rng.integers(0, 3)), jitter=True,
                      nulls=nulls)
    return make


def _build():
    cases = []

    def add(*a, **k):
        cases.append(Case(*a, **k))
    add('ties', 'ties/2x2', 90, 90, 40, 16, _ties, seed=TIES_SEEDS[0])
    add('ties', 'ties/3x3', 110, 110, 40, 16, _ties, seed=TIES_SEEDS[1])
    for o in (2, 3, 7, 16, 17, 1):
        add('midline', 'midline/ov%d' % o, 75, 78, 36, o, _midline, seed=100 + o)
    add('both_strips', 'both_strips/3x3', 118, 121, 44, 16, _both, seed=7)
    add('shapes', 'shapes/2x2', 150, 141, 64, 16, _shapes, seed=11)
    add('lane_edges', 'lane_edges/w70', 141, 145, 70, 16, _lane_edges, seed=21)
    add('lane_edges', 'lane_edges/w130', 262, 265, 130, 24, _lane_edges, seed=22)
    add('outside_owner', 'outside_owner/2x2', 100, 104, 48, 16, _outside_owner, seed=31)
    add('dense_pairs', 'dense_pairs/2x2', 112, 118, 56, 16, _dense_pairs, seed=41)
    add('many_segments', 'many_segments/2x2', 276, 276, 100, 16, _many, seed=51)
    add('grids', 'grids/1xN', 40, 150, 48, 8, _jitter(5, 6, 0.02), seed=61)
    add('grids', 'grids/Nx1', 150, 40, 48, 8, _jitter(6, 5, 0.02), seed=62)
    add('grids', 'grids/grown', 139, 151, 40, 12, _jitter(7, 7, 0.02), seed=63)
    rng = np.random.default_rng(2024)
    for s in range(20):
        tile = int(rng.choice([32, 40, 48]))
        ov = int(rng.choice([3, 4, 7, 8, 16]))
        (nr, nc) = (int(rng.integers(60, 141)), int(rng.integers(60, 141)))
        add('random', 'random/%02d' % s, nr, nc, tile, ov, _jitter(3 + s % 4, 3 + (s // 4) % 4, 0.03), seed=1000 + s)
    return cases


TIES_SEEDS = (3, 4)
_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


GROUPS = ['ties', 'midline', 'both_strips', 'shapes', 'lane_edges', 'outside_owner', 'dense_pairs',
          'many_segments', 'grids', 'random']


def group(name):
    return [c for c in all_cases() if c.group == name]


def case(name):
    return [c for c in all_cases() if c.name == name][0]


# ----------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------
def hash64(k):
    """the pair table's hash (stitch.h), on a 64-bit key"""
    M = (1 << 64) - 1
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M
    k ^= k >> 33
    return k & 0xFFFFFFFF


def table_size(case, ys, xs, has_top, has_left, cross_px):
    """slots of the chain step's pair table for a tile whose strips have cross_px crossing pixels"""
    o = case.overlap
    (an_rows, an_cols) = (min(o, ys), min(o, xs))
    m = 0
    if has_top:
        m = min(cross_px[0], an_rows * xs)
    if has_left:
        m = max(m, min(cross_px[1], ys * an_cols))
    h = 1024
    while h < 2 * m:
        h <<= 1
    return h


class TileResult(object):
    pass


class StitchResult(object):
    pass


def _new_census():
    keys = ('modes', 'ties', 'ties_zero', 'ties3', 'tie_win_hi_slot', 'tie_win_lo_slot', 'overrides', 'cross_both',
            'cross_top_only', 'cross_left_only', 'outside_new', 'k_ne_r', 'max_local', 'max_ids_per_patch',
            'row_continuations', 'max_cross_px', 'dense_strips')
    cen = {k: 0 for k in keys}
    for s in ('top', 'left'):
        for k in ('ends_before', 'starts_at', 'spans', 'crossing'):
            cen['%s_%s' % (s, k)] = 0
    cen['k_ne_r_tiles'] = []
    return cen


def _recode_shared(tile, B, srows, scols, horizontal, nseg, cen, ties):
    """recodeSharedSegments (tiling.py:1128-1203) with crossesMidline (:1271-1306): {segment: mode} of the
    segments of the strip tile[:srows, :scols] that cross its midline, the crossing mask and the number of
    strip pixels that belong to a crossing segment."""
    A = tile[:srows, :scols]                            # tiling.py:1101-1102
    assert B.shape == A.shape
    name = 'top' if horizontal else 'left'
    mid = int((srows if horizontal else scols) / 2)     # tiling.py:1297 / :1300
    (rr, cc) = np.nonzero(A)                            # every labelled pixel (:1170-1175), raster order
    lab = A[rr, cc]
    v = rr if horizontal else cc
    mn = np.full(nseg, BIG, dtype=np.int64)
    mx = np.full(nseg, -1, dtype=np.int64)
    np.minimum.at(mn, lab, v)
    np.maximum.at(mx, lab, v)
    cross = (mn < mid) & (mx >= mid)                    # tiling.py:1303-1306
    present = mx >= 0
    cen[name + '_ends_before'] += int((present & (mx == mid - 1)).sum())
    cen[name + '_starts_at'] += int((present & (mn == mid)).sum())
    cen[name + '_spans'] += int((present & (mn == mid - 1) & (mx == mid)).sum())
    cen[name + '_crossing'] += int(cross.sum())
    sel = cross[lab]
    cross_px = int(sel.sum())
    (lab, b, lin) = (lab[sel], B[rr[sel], cc[sel]], (rr[sel] * scols + cc[sel]))
    # runs of one (segment, neighbour id) key that go on from a strip row's end into the next row's start
    # inside one wavefront of the pair-count kernels (64 consecutive strip pixels)
    key = lab.astype(np.uint64) << np.uint64(32) | b.astype(np.uint64)
    nxt = (lin[1:] == lin[:-1] + 1) & (key[1:] == key[:-1]) & (lin[1:] % scols == 0) & (lin[1:] % 64 != 0)
    cen['row_continuations'] += int(nxt.sum())
    if cross_px and len(np.unique(key)) == cross_px:
        cen['dense_strips'] += 1
    cen['max_cross_px'] = max(cen['max_cross_px'], cross_px)
    order = np.argsort(lab, kind='stable')              # the pixels of a segment together (:1189)
    (lab, b) = (lab[order], b[order])
    (ids, start) = np.unique(lab, return_index=True)
    ends = np.append(start[1:], len(lab))
    modes = {}
    for (s, a, e) in zip(ids.tolist(), start.tolist(), ends.tolist()):
        (vals, cnt) = np.unique(b[a:e], return_counts=True)
        winners = vals[cnt == cnt.max()]
        modes[s] = int(winners[0])                      # scipy.stats.mode: the smallest of the most frequent (:1194)
        cen['modes'] += 1
        if len(winners) > 1:
            cen['ties'] += 1
            cen['ties_zero'] += int(winners[0] == 0)
            cen['ties3'] += int(len(winners) >= 3)
            ties.append((s, int(winners[0]), int(winners[1])))
    return modes, cross, cross_px


def _recode_tile(case, col, row, tile, top_b, left_b, base, cen):
    """recodeTile (tiling.py:1066-1126) + relabelSegments (:1205-1269) for one tile -> TileResult"""
    o = case.overlap
    (ys, xs) = tile.shape
    (top, bottom, left, right, _x, _y) = case.window(col, row)
    nseg = int(tile.max()) + 1
    res = TileResult()
    recode = {}
    (ties_t, ties_l) = ([], [])
    res.cross_top = np.zeros(nseg, dtype=bool)
    res.cross_left = np.zeros(nseg, dtype=bool)
    res.cross_px = [0, 0]
    (mt, ml) = ({}, {})
    if top_b is not None:                               # tiling.py:1107-1113
        (mt, res.cross_top, res.cross_px[0]) = _recode_shared(tile, top_b, min(o, ys), xs, True, nseg, cen, ties_t)
        recode.update(mt)
    if left_b is not None:                              # tiling.py:1115-1121: the same dict, so left overrides
        (ml, res.cross_left, res.cross_px[1]) = _recode_shared(tile, left_b, ys, min(o, xs), False, nseg, cen, ties_l)
        recode.update(ml)
    (res.modes_top, res.modes_left) = (mt, ml)
    both = res.cross_top & res.cross_left
    cen['cross_both'] += int(both.sum())
    cen['cross_top_only'] += int((res.cross_top & ~res.cross_left).sum())
    cen['cross_left_only'] += int((res.cross_left & ~res.cross_top).sum())
    cen['overrides'] += sum(1 for s in np.nonzero(both)[0].tolist() if mt[s] != ml[s])
    # which of a tie's two smallest winners sits in the higher slot of the device's pair table
    hmask = table_size(case, ys, xs, top_b is not None, left_b is not None, res.cross_px) - 1
    for (s, w, l) in ties_t + ties_l:
        (hw, hl) = (hash64(s << 32 | w) & hmask, hash64(s << 32 | l) & hmask)
        cen['tie_win_hi_slot'] += int(hw > hl)
        cen['tie_win_lo_slot'] += int(hw < hl)
    # relabelSegments: every id in ascending order (makeSegmentLocations inserts them so, :1245-1250)
    (rr, cc) = np.nonzero(tile)
    lab = tile[rr, cc]
    segtop = np.full(nseg, BIG, dtype=np.int64)
    segleft = np.full(nseg, BIG, dtype=np.int64)
    np.minimum.at(segtop, lab, rr)                      # tiling.py:1256-1257
    np.minimum.at(segleft, lab, cc)
    assert (segtop[1:] != BIG).all(), 'an id without pixels: the reference raises on it'
    in_dict = np.zeros(nseg, dtype=bool)
    lut = np.zeros(nseg, dtype=np.int64)
    for (s, v) in recode.items():                       # tiling.py:1252-1253
        in_dict[s] = True
        lut[s] = v
    own = (~in_dict & (segleft >= left) & (segtop >= top) & (segleft < right) & (segtop < bottom))     # :1264-1265
    own[0] = False
    lut[own] = base + np.cumsum(own)[own]               # newSegId += 1, :1266-1267
    res.lut = lut.astype(np.uint32)
    res.recoded = res.lut[tile]
    res.segtop = segtop
    res.segleft = segleft
    res.in_trim = np.bincount(tile[top:bottom, left:right].ravel(), minlength=nseg) > 0
    res.in_trim[0] = False
    res.own = own
    res.K = int(own.sum())
    shown = own & res.in_trim
    res.R = int((lut[shown] - base).max()) if shown.any() else 0
    res.base = base
    cen['outside_new'] += int((own & ~res.in_trim).sum())
    if res.K != res.R:
        cen['k_ne_r'] += 1
        cen['k_ne_r_tiles'].append((col, row))
    cen['max_local'] = max(cen['max_local'], nseg - 1)
    # ids per 32-row x 64-column patch (the LDS table of the per-segment reductions holds 128)
    for r0 in range(0, ys, 32):
        for c0 in range(0, xs, 64):
            u = np.unique(tile[r0:r0 + 32, c0:c0 + 64])
            cen['max_ids_per_patch'] = max(cen['max_ids_per_patch'], int((u != 0).sum()))
    return res


def model_stitch(case, simple=False):
    """stitchTiles (tiling.py:950-1064) over the case's tiles -> StitchResult with mosaic, maxSegId, hist,
    census and tiles[(col, row)] = TileResult (recoded, right, bottom, lut, cross_top, cross_left, in_trim,
    segtop, segleft, cross_px, K, R, base)."""
    key = bool(simple)
    if key in case._model:
        return case._model[key]
    o = case.overlap
    out = StitchResult()
    out.mosaic = np.zeros((case.nr, case.nc), dtype=np.uint32)
    out.tiles = {}
    cen = _new_census()
    max_seg = 0                                         # tiling.py:979
    for (col, row) in case.order():
        tile = case.tiles[(col, row)]
        (top, bottom, left, right, xout, yout) = case.window(col, row)
        if simple:                                      # tiling.py:1024-1027
            res = TileResult()
            nseg = int(tile.max()) + 1
            res.lut = np.where(np.arange(nseg) == 0, 0, np.arange(nseg) + max_seg).astype(np.uint32)
            res.recoded = res.lut[tile]
            (rr, cc) = np.nonzero(tile)
            res.segtop = np.full(nseg, BIG, dtype=np.int64)
            res.segleft = np.full(nseg, BIG, dtype=np.int64)
            np.minimum.at(res.segtop, tile[rr, cc], rr)
            np.minimum.at(res.segleft, tile[rr, cc], cc)
            res.in_trim = np.bincount(tile[top:bottom, left:right].ravel(), minlength=nseg) > 0
            res.in_trim[0] = False
            res.cross_top = res.cross_left = np.zeros(nseg, dtype=bool)
            res.cross_px = [0, 0]
            res.base = max_seg
        else:
            top_b = out.tiles[(col, row - 1)].bottom if row > 0 else None
            left_b = out.tiles[(col - 1, row)].right if col > 0 else None
            res = _recode_tile(case, col, row, tile, top_b, left_b, max_seg, cen)
        trimmed = res.recoded[top:bottom, left:right]   # tiling.py:1032-1033
        out.mosaic[yout:yout + trimmed.shape[0], xout:xout + trimmed.shape[1]] = trimmed
        res.right = res.recoded[:, -o:].copy() if col != case.ntc - 1 else None      # tiling.py:1037-1040
        res.bottom = res.recoded[-o:, :].copy() if row != case.ntr - 1 else None
        max_seg = max(max_seg, int(trimmed.max()))      # tiling.py:1042-1043
        out.tiles[(col, row)] = res
    out.maxSegId = max_seg
    out.hist = np.bincount(out.mosaic.ravel(), minlength=max_seg + 1).astype(np.uint32)
    out.hist[0] = 0                                     # HistogramAccumulator: the null id is not counted
    out.census = cen
    case._model[key] = out
    return out


def group_census(name):
    tot = _new_census()
    for c in group(name):
        cen = model_stitch(c).census
        for (k, v) in cen.items():
            if k.startswith('max_'):
                tot[k] = max(tot[k], v)
            elif k == 'k_ne_r_tiles':
                tot[k] = tot[k] + [(c.name,) + t for t in v]
            else:
                tot[k] += v
    return tot


def census_table():
    rows = ['    %-14s %7s %6s %5s %7s %6s %9s %5s %5s %5s %6s %9s' % (
        'group', 'tilings', 'modes', 'ties', '0 wins', '3-way', 'hi / lo', 'ovr', 'out', 'K!=R', 'max id', 'cross px')]
    for g in GROUPS:
        t = group_census(g)
        rows.append('    %-14s %7d %6d %5d %7d %6d %9s %5d %5d %5d %6d %9d' % (
            g, len(group(g)), t['modes'], t['ties'], t['ties_zero'], t['ties3'],
            '%d / %d' % (t['tie_win_hi_slot'], t['tie_win_lo_slot']), t['overrides'], t['outside_new'], t['k_ne_r'],
            t['max_local'], t['max_cross_px']))
    return '\n'.join(rows)


if __name__ == '__main__':                  # python -m tests.stitch_cases: the table of the docstring
    print(census_table())
