"""The definition of the segment-neighbour table in numpy, and the label rasters the tests put through it.

Two pixels are adjacent when they are E or S neighbours (8-connected: SE and SW as well); every adjacent pair
with labels a != b, both non-zero, adds 1 to the border length of (a, b) and of (b, a).  The table is CSR over
the ids 0 .. maxSegId."""
import numpy as np

EXAMPLE = np.array([[1, 1, 2], [1, 3, 2], [0, 3, 3]], dtype=np.uint32)
EXAMPLE_OFFSETS = [0, 0, 2, 4, 6]
EXAMPLE_NEIGHBOURS = [2, 3, 1, 3, 1, 2]
EXAMPLE_LENGTHS = {True: [1, 2, 1, 2, 2, 2], False: [2, 4, 2, 4, 4, 4]}


def reference_neighbours(seg, fourConnected=True, maxSegId=None):
    """(offsets int64 [maxSegId + 2], neighbours uint32, borderLengths int64)"""
    seg = np.asarray(seg)
    assert seg.ndim == 2 and seg.dtype == np.uint32
    if maxSegId is None:
        maxSegId = int(seg.max()) if seg.size else 0
    pairs = [(seg[:, :-1], seg[:, 1:]), (seg[:-1], seg[1:])]
    if not fourConnected:
        pairs += [(seg[:-1, :-1], seg[1:, 1:]), (seg[:-1, 1:], seg[1:, :-1])]
    a = np.concatenate([p[0].ravel() for p in pairs]).astype(np.uint64)
    b = np.concatenate([p[1].ravel() for p in pairs]).astype(np.uint64)
    keep = (a != b) & (a != 0) & (b != 0)
    (a, b) = (a[keep], b[keep])
    (u, cnt) = np.unique(np.concatenate([(a << np.uint64(32)) | b, (b << np.uint64(32)) | a]), return_counts=True)
    offsets = np.zeros(maxSegId + 2, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount((u >> np.uint64(32)).astype(np.int64), minlength=maxSegId + 1))
    return (offsets, (u & np.uint64(0xFFFFFFFF)).astype(np.uint32), cnt.astype(np.int64))


def random_labels(shape, top, seed):
    """uniform labels 0 .. top"""
    return np.random.default_rng(seed).integers(0, top + 1, size=shape, dtype=np.uint32)


OFF_GRID_SHAPES = [(1, 1), (1, 257), (257, 1), (2, 2), (33, 65), (65, 129)]


def every_pixel_its_own():
    return np.arange(1, 70 * 130 + 1, dtype=np.uint32).reshape(70, 130)


def half_planes():
    seg = np.ones((300, 300), dtype=np.uint32)
    seg[150:] = 2
    return seg


def stripes():
    seg = np.empty((257, 300), dtype=np.uint32)
    seg[:, 0::2] = 1
    seg[:, 1::2] = 2
    return seg


def hot_segment():
    seg = np.ones((300, 300), dtype=np.uint32)
    (ys, xs) = np.meshgrid(np.arange(1, 300, 2), np.arange(1, 300, 2), indexing='ij')
    seg[ys, xs] = np.arange(2, 2 + ys.size, dtype=np.uint32).reshape(ys.shape)
    return seg


SPARSE_IDS = np.array([0, 5, 70000, 1 << 20], dtype=np.uint32)
SPARSE_MAX = (1 << 20) + 3


def sparse_ids():
    return SPARSE_IDS[np.random.default_rng(5).integers(0, 4, size=(90, 140))]


def enclosed_by_zeros():
    seg = np.zeros((40, 70), dtype=np.uint32)
    seg[10:20, 10:30] = 3          # touches nothing but zeros
    seg[25:35, 40:50] = 1
    seg[25:35, 50:66] = 2          # 1 and 2 touch each other
    return seg


# ---- what the patches hand to the sort ------------------------------------------------------------------------
PATCH_ROWS = 32
PATCH_COLS = 64
TABLE_SLOTS = 1024


def patch_records(seg, fourConnected=True, rowsPerBlock=None):
    """(per, total): what the patch kernel's definition (the header comment of csrc/neighbours.h) makes of a raster.

    The raster is cut into row blocks of rowsPerBlock rows (None: one block) and every block into patches of
    32 x 64 pixels from its own first row.  A differing pair belongs to the patch of its upper pixel (for E: the
    left one); its other pixel may lie in the patch's rim, below only where the raster has another row.  The pairs
    of one patch row and one direction form runs: maximal stretches of adjacent columns of the patch that hold the
    same (min, max) pair; a column without a pair, or the patch's first column, starts a new stretch.

    per: int64 [patches, 3], (distinct pairs D, runs R, pairs P) of every patch, blocks from the top, the patches
    of a block row-major.  total: the records, D of a patch that has at most 1024 distinct pairs, else R."""
    seg = np.asarray(seg)
    assert seg.ndim == 2 and seg.dtype == np.uint32
    (nrows, ncols) = seg.shape
    if nrows == 0 or ncols == 0:
        return (np.zeros((0, 3), dtype=np.int64), 0)
    rpb = nrows if rowsPerBlock is None else max(1, min(nrows, int(rowsPerBlock)))
    pcols = -(-ncols // PATCH_COLS)
    ys = np.arange(nrows)
    inBlock = ys % rpb
    # patch rows of the blocks before a row's block (all full blocks), then the patch row inside the block
    patchRow = (ys // rpb) * (-(-rpb // PATCH_ROWS)) + inBlock // PATCH_ROWS
    npatch = (int(patchRow[-1]) + 1) * pcols
    patch = patchRow[:, None] * pcols + (np.arange(ncols) // PATCH_COLS)[None, :]
    firstLane = np.arange(ncols) % PATCH_COLS == 0
    dirs = [(0, 1), (1, 0)] + ([] if fourConnected else [(1, 1), (1, -1)])
    (keys, keyPatch) = ([], [])
    runs = np.zeros(npatch, dtype=np.int64)
    pairs = np.zeros(npatch, dtype=np.int64)
    for (dy, dx) in dirs:
        other = np.zeros_like(seg)              # the label at (y + dy, x + dx), 0 past the raster's end
        src = seg[dy:, max(dx, 0):ncols + min(dx, 0)]
        other[:nrows - dy, max(-dx, 0):ncols - max(dx, 0)] = src
        valid = (seg != 0) & (other != 0) & (seg != other)
        lo = np.where(valid, np.minimum(seg, other), 0).astype(np.uint64)
        hi = np.where(valid, np.maximum(seg, other), 0).astype(np.uint64)
        key = (lo << np.uint64(32)) | hi        # 0 where there is no pair
        head = valid.copy()
        head[:, 1:] &= (key[:, 1:] != key[:, :-1]) | firstLane[None, 1:]
        runs += np.bincount(patch[head], minlength=npatch)
        pairs += np.bincount(patch[valid], minlength=npatch)
        keys.append(key[valid])
        keyPatch.append(patch[valid])
    keys = np.concatenate(keys)
    keyPatch = np.concatenate(keyPatch)
    distinct = np.zeros(npatch, dtype=np.int64)
    if len(keys):
        (u, inv) = np.unique(keys, return_inverse=True)
        up = np.unique(keyPatch.astype(np.int64) * len(u) + inv.reshape(-1))
        distinct = np.bincount(up // len(u), minlength=npatch)
    per = np.stack([distinct, runs, pairs], axis=1).astype(np.int64)
    total = int(np.where(distinct <= TABLE_SLOTS, distinct, runs).sum())
    return (per, total)


def patch_record_counts(per):
    """records of every patch of patch_records' first result"""
    return np.where(per[:, 0] <= TABLE_SLOTS, per[:, 0], per[:, 1])


# ---- cases that reach the paths behind a threshold ---------------------------------------------------------------
TABLE_FILL_WINDOW = {True: (20, 30), False: (12, 26)}


def _window_patch(m, four, isolated=0):
    """a 32 x 64 patch of 1s; the first m pixels (row-major) of the window at (1, 1) and `isolated` pixels on odd
    rows and the even columns 34 .. 62 have labels of their own, from 2"""
    (wh, ww) = TABLE_FILL_WINDOW[four]
    p = np.ones((PATCH_ROWS, PATCH_COLS), dtype=np.uint32)
    k = np.arange(m)
    p[1 + k // ww, 1 + k % ww] = 2 + k
    k = np.arange(isolated)
    p[1 + 2 * (k // 15), 34 + 2 * (k % 15)] = 2 + m + k
    return p


def table_fill_parts(n, four):
    """(window pixels m, isolated pixels) of table_fill: m is the largest count of window pixels that gives at most n
    distinct pairs, the isolated pixels add one pair (1, own) each"""
    (wh, ww) = TABLE_FILL_WINDOW[four]
    best = None
    for m in range(wh * ww + 1):
        d = int(patch_records(_window_patch(m, four), four)[0][0, 0])
        if d <= n:
            best = (m, n - d)
    assert best is not None and best[1] <= 15 * 16
    return best


def table_fill(n, four):
    """a 96 x 192 raster of 1s whose patch (1, 1) holds exactly n distinct pairs, all of them inside the patch, and
    more runs than distinct pairs"""
    (m, isolated) = table_fill_parts(n, four)
    seg = np.ones((3 * PATCH_ROWS, 3 * PATCH_COLS), dtype=np.uint32)
    seg[PATCH_ROWS:2 * PATCH_ROWS, PATCH_COLS:2 * PATCH_COLS] = _window_patch(m, four, isolated)
    return seg


def pair_home(a, b):
    """the slot of a patch's 1024-slot table where the pair (a, b), a < b, is looked for first: nbr_hash of
    csrc/neighbours.h in its 32-bit arithmetic"""
    m = np.uint64(0xFFFFFFFF)
    (a, b) = (np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64))
    h = ((a * np.uint64(0x9E3779B1)) & m) ^ ((b * np.uint64(0x85EBCA6B)) & m)
    h ^= h >> np.uint64(15)
    return ((((h * np.uint64(2654435761)) & m) >> np.uint64(16)) & np.uint64(TABLE_SLOTS - 1)).astype(np.int64)


TABLE_WRAP_HOME = 5


def table_wrap_chains():
    """16 chains of 65 ascending labels, all different: two labels next to each other in a chain are a pair whose
    home is slot TABLE_WRAP_HOME.  int64 [16, 65]"""
    chains = np.empty((PATCH_ROWS // 2, PATCH_COLS + 1), dtype=np.int64)
    last = 0
    for chain in chains:
        chain[0] = last = last + 1
        for i in range(1, len(chain)):
            while True:
                cand = np.arange(last + 1, last + 1 + 8192)
                hit = np.flatnonzero(pair_home(chain[i - 1], cand) == TABLE_WRAP_HOME)
                if len(hit):
                    break
                last = int(cand[-1])
            chain[i] = last = int(cand[hit[0]])
    return chains


def table_wrap():
    """a 96 x 192 raster of 0s whose patch (1, 1) holds exactly 1024 distinct pairs that all have the SAME home slot,
    and 1025 runs.  Linear probing then puts them in 1024 slots in a row, so whichever pair arrives last finds its
    slot only with the 1024th probe, the last one of its trip round the table -- with any other set of 1024 pairs
    that depends on the order of arrival, if it happens at all.

    Every second row of the patch holds a chain of table_wrap_chains() from its first column to the first column of
    the next patch, zeros between the rows: 16 x 64 E pairs, nothing else.  The pixel below the last chain's 64th
    label repeats its 63rd: the S pair there is the chain's 63rd pair in a run of its own (with 8-connectivity the
    65th label, which lies in the next patch, gains a SW pair that belongs to that patch)."""
    chains = table_wrap_chains()
    seg = np.zeros((3 * PATCH_ROWS, 3 * PATCH_COLS), dtype=np.uint32)
    seg[PATCH_ROWS:2 * PATCH_ROWS:2, PATCH_COLS:2 * PATCH_COLS + 1] = chains
    seg[2 * PATCH_ROWS - 1, 2 * PATCH_COLS - 1] = chains[-1, PATCH_COLS - 2]
    return seg


def zone_stripes():
    """one-pixel stripes of two labels per 64-column zone: nine pairs, each in every row"""
    x = np.arange(313, dtype=np.uint32)
    return np.ascontiguousarray(np.broadcast_to(1 + 2 * (x // 64) + x % 2, (203, 313)))


def hot_segment_top():
    """hot_segment() with the background as the LARGEST label: all of its 22 500 neighbours are smaller"""
    seg = hot_segment()
    seg[seg == 1] = int(seg.max()) + 1
    return seg


def calm_then_busy():
    """64 rows of 8 x 8 blocks, then 32 rows of pixels with labels of their own: a row block that needs many times
    the records of the blocks before it"""
    (y, x) = np.meshgrid(np.arange(96, dtype=np.uint32), np.arange(128, dtype=np.uint32), indexing='ij')
    seg = 1 + (y // 8) * 16 + x // 8
    seg[64:] = 1000 + np.arange(32 * 128, dtype=np.uint32).reshape(32, 128)
    return seg.astype(np.uint32)


WIDE_IDS = np.array([0, 5, 70000, (1 << 24) + 9], dtype=np.uint32)
WIDE_MAX = (1 << 24) + 12


def wide_ids():
    """sparse_ids() with a largest label past 2^24: four passes of the radix sort"""
    return WIDE_IDS[np.random.default_rng(5).integers(0, 4, size=(90, 140))]
