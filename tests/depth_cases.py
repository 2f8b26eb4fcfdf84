"""The cases of tests/test_gpu_depths.py -- depths.calcSegmentDepths (pyshepseg_amd/csrc/segdepth.h) -- with the numpy
model of its columns and the literal definition of depth2.

Importable without a GPU: tests/test_depth_cases_host.py holds the model to the definition and counts what the cases
reach.  Everything the kernels decide is integer work: results are compared with numpy.array_equal.

depth2 of a pixel of label L != 0 is the smallest squared distance to a position that is outside the raster or of
another label (0 included); 0 where the label is 0.  ``brute_depth2`` is that sentence.  ``reference_depth2`` is the
two-step form: g(y, x) = min(y - top + 1, bottom - y + 1) over the vertical run of the pixel's label, and with l .. r
the horizontal run of its label depth2 = min((x - l + 1)^2, (r + 1 - x)^2, min over x' in l .. r of (x - x')^2 +
g(y, x')^2).

The kernels' sizes, restated here and held to the header by tests/test_depth_cases_host.py: a column band of BAND rows;
a window tile of TH rows x TW columns whose pixels look HALO columns to either side; a reduction patch of PH rows x TW
columns with a table of SLOTS labels.  ``window_deferred`` is the window's rule: a labelled pixel is deferred to the
envelope when its label holds HALO columns to either side and after the offsets 1 .. HALO - 1 the best is still above
HALO^2.
"""
import functools

import numpy as np

HALO = 32
BAND = 32
TW = 64
TH = 16
PH = 32
SLOTS = 512
CORES = 8
HEADER_NAMES = {'HALO': 'DEPTH_HALO', 'BAND': 'DEPTH_BAND', 'TW': 'DEPTH_TW', 'TH': 'DEPTH_TH', 'PH': 'DEPTH_PH',
                'SLOTS': 'DEPTH_SLOTS', 'CORES': 'DEPTH_CORES'}

COUNTS = ('maxDepth2', 'interiorRow', 'interiorCol', 'sumDepth2')
DERIVED = ('maxDepth', 'meanDepth2', 'depthRatio')


# ---- the definition and the model -----------------------------------------------------------------------------------
def brute_depth2(seg):
    """the definition: for every labelled pixel the minimum over all foreign positions of the raster and of a ring of
    outside positions round it (an outside position farther out is farther from every pixel than the ring position
    its coordinates clamp to); for rasters up to a few dozen pixels a side"""
    seg = np.asarray(seg)
    (h, w) = seg.shape
    out = np.zeros((h, w), dtype=np.uint32)
    if h == 0 or w == 0:
        return out
    padded = np.zeros((h + 2, w + 2), dtype=np.int64)
    padded[1:-1, 1:-1] = seg
    outside = np.ones((h + 2, w + 2), dtype=bool)
    outside[1:-1, 1:-1] = False
    (qy, qx) = np.mgrid[-1:h + 1, -1:w + 1]
    for y in range(h):
        for x in range(w):
            if seg[y, x] == 0:
                continue
            foreign = outside | (padded != seg[y, x])
            d2 = (qy - y) ** 2 + (qx - x) ** 2
            out[y, x] = d2[foreign].min()
    return out


def column_distance(seg):
    """g: the distance along the column to the nearest pixel of another label or the outside of the raster, int64"""
    seg = np.asarray(seg)
    (h, w) = seg.shape
    down = np.ones((h, w), dtype=np.int64)
    up = np.ones((h, w), dtype=np.int64)
    for y in range(1, h):
        down[y] = np.where(seg[y] == seg[y - 1], down[y - 1] + 1, 1)
    for y in range(h - 2, -1, -1):
        up[y] = np.where(seg[y] == seg[y + 1], up[y + 1] + 1, 1)
    return np.minimum(down, up)


def _row_runs(row):
    """(first, last) column of every pixel's run of equal labels in the row"""
    w = len(row)
    x = np.arange(w)
    start = np.ones(w, dtype=bool)
    start[1:] = row[1:] != row[:-1]
    first = np.maximum.accumulate(np.where(start, x, 0))
    end = np.ones(w, dtype=bool)
    end[:-1] = row[1:] != row[:-1]
    last = np.minimum.accumulate(np.where(end, x, w)[::-1])[::-1]
    return first, last


def reference_depth2(seg):
    """depth2 by the two-step form, one row at a time over a (W, W) array of offsets^2 + g^2 masked to the row run"""
    seg = np.asarray(seg)
    (h, w) = seg.shape
    out = np.zeros((h, w), dtype=np.uint32)
    if h == 0 or w == 0:
        return out
    g = column_distance(seg)
    x = np.arange(w, dtype=np.int64)
    off2 = (x[:, None] - x[None, :]) ** 2
    for y in range(h):
        (first, last) = _row_runs(seg[y])
        same = (x[None, :] >= first[:, None]) & (x[None, :] <= last[:, None])
        cand = np.where(same, off2 + (g[y] ** 2)[None, :], np.iinfo(np.int64).max).min(axis=1)
        d2 = np.minimum(np.minimum((x - first + 1) ** 2, (last + 1 - x) ** 2), cand)
        out[y] = np.where(seg[y] != 0, d2, 0)
    return out


def rectangle_depth2(h, w):
    """the closed form for a rectangle of one label whose four sides are foreign"""
    (y, x) = np.mgrid[0:h, 0:w]
    m = np.minimum(np.minimum(y + 1, h - y), np.minimum(x + 1, w - x)).astype(np.int64)
    return (m * m).astype(np.uint32)


def columns_from_depth2(seg, depth2, coreAreas=(), origin=(0, 0), maxSegId=None, missing=-9999):
    """the columns of depths.calcSegmentDepths from a depth2 raster: a dictionary; ``coreAreas`` pairs (name, depth)"""
    seg = np.asarray(seg)
    S = int(seg.max()) if maxSegId is None and seg.size else (0 if maxSegId is None else int(maxSegId))
    lab = seg.ravel().astype(np.int64)
    d2 = np.asarray(depth2).ravel().astype(np.int64)
    order = np.argsort(lab, kind='stable')                  # row-major order within every label
    (slab, sd2) = (lab[order], d2[order])
    area = np.bincount(lab, minlength=S + 1)[:S + 1].astype(np.int64)
    area[0] = 0
    cols = {k: np.zeros(S + 1, dtype=np.int64) for k in COUNTS}
    for (name, _depth) in coreAreas:
        cols[name] = np.zeros(S + 1, dtype=np.int64)
    ids = np.flatnonzero(area > 0)
    if len(ids):
        starts = np.searchsorted(slab, ids, side='left')
        mx = np.maximum.reduceat(sd2, starts)
        cols['maxDepth2'][ids] = mx
        cols['sumDepth2'][ids] = np.add.reduceat(sd2, starts)
        per_pixel_max = np.zeros(S + 1, dtype=np.int64)
        per_pixel_max[ids] = mx
        inside = slab <= S
        is_max = np.zeros(len(slab), dtype=bool)
        is_max[inside] = sd2[inside] == per_pixel_max[slab[inside]]
        firstpos = np.minimum.reduceat(np.where(is_max, order, lab.size), starts)
        w = seg.shape[1]
        cols['interiorRow'][ids] = origin[0] + firstpos // w
        cols['interiorCol'][ids] = origin[1] + firstpos % w
        for (name, depth) in coreAreas:
            q = int(np.floor(float(depth) * float(depth)))
            cols[name][ids] = np.add.reduceat((sd2 > q).astype(np.int64), starts)
    has = area > 0
    a = area[has].astype(np.float64)
    for k in DERIVED:
        cols[k] = np.full(S + 1, float(missing), dtype=np.float64)
    cols['maxDepth'][has] = np.sqrt(cols['maxDepth2'][has].astype(np.float64))
    cols['meanDepth2'][has] = cols['sumDepth2'][has].astype(np.float64) / a
    cols['depthRatio'][has] = np.pi * cols['maxDepth2'][has].astype(np.float64) / a
    return cols


def reference_depths(seg, coreAreas=(), origin=(0, 0), maxSegId=None, missing=-9999):
    """(columns, depth2) of the model"""
    d2 = reference_depth2(seg)
    return columns_from_depth2(seg, d2, coreAreas, origin, maxSegId, missing), d2


def window_deferred(seg, depth_g=None):
    """the pixels the window of the row step defers, a boolean raster: labelled, the own label at all offsets 1 .. HALO
    on both sides, and min(g^2, min over d < HALO of d^2 + min(g(x - d), g(x + d))^2) > HALO^2"""
    seg = np.asarray(seg)
    (h, w) = seg.shape
    g = column_distance(seg) if depth_g is None else depth_g
    g = np.minimum(g, 65535)
    out = np.zeros((h, w), dtype=bool)
    x = np.arange(w)
    for y in range(h):
        (first, last) = _row_runs(seg[y])
        roomy = (seg[y] != 0) & (x - first >= HALO) & (last - x >= HALO)
        best = g[y] ** 2
        for d in range(1, HALO):
            left = np.full(w, 65535, dtype=np.int64)
            right = np.full(w, 65535, dtype=np.int64)
            left[d:] = g[y, :-d]
            right[:-d] = g[y, d:]
            best = np.minimum(best, d * d + np.minimum(left, right) ** 2)
        out[y] = roomy & (best > HALO * HALO)
    return out


# ---- builders ---------------------------------------------------------------------------------------------------------
def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def blocky(shape, cell, top, seed, zero=True):
    """random labels (0 .. top, or 1 .. top) in cells of ``cell`` x ``cell`` pixels, cut to ``shape``"""
    (h, w) = shape
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0 if zero else 1, top + 1, size=(-(-h // cell), -(-w // cell)), dtype=np.uint32)
    return u32(np.kron(coarse, np.ones((cell, cell), dtype=np.uint32))[:h, :w])


def blown_up(seed):
    """a raster for the definition: up to 5 x 5 cells of 1 .. 4 labels and label 0, blown up by 1 .. 3"""
    rng = np.random.default_rng(seed)
    (h, w) = (int(rng.integers(1, 6)), int(rng.integers(1, 6)))
    top = int(rng.integers(1, 5))
    f = int(rng.integers(1, 4))
    coarse = rng.integers(0, top + 1, size=(h, w), dtype=np.uint32)
    return u32(np.kron(coarse, np.ones((f, f), dtype=np.uint32)))


# 1 x 1, a row, a column, 2 x 2; then heights and widths one below, at and one above the window tile's rows (TH), the
# band and patch rows (BAND = PH), the halo and the tile's columns (TW), and two tiles
GEOMETRY = [(1, 1), (1, 2 * TW + 3), (2 * BAND + 3, 1), (2, 2),
            (TH - 1, HALO - 1), (TH, HALO), (TH + 1, HALO + 1),
            (BAND - 1, TW - 1), (BAND, TW), (BAND + 1, TW + 1),
            (2 * BAND - 1, 2 * TW + 1), (2 * BAND, 2 * TW), (2 * BAND + 1, 2 * TW - 1),
            (3 * BAND + 5, HALO + TW + 1)]


def geometry_rasters(shape):
    """the rasters of one shape: cells of 1 (single pixels), 5 and 23 pixels, with and without label 0"""
    out = []
    for (k, (cell, top)) in enumerate(((1, 6), (5, 40), (23, 3))):
        for zero in (True, False):
            out.append(blocky(shape, cell, top, 100 * shape[0] + shape[1] + 7 * k + zero, zero))
    return out


def one_label(h, w, label=1):
    return np.full((h, w), label, dtype=np.uint32)


def square_of_depth(depth, odd=True):
    """the one-label square whose deepest pixel has that depth: side 2 depth - 1 (one deepest pixel) or 2 depth (four)"""
    side = 2 * depth - 1 if odd else 2 * depth
    return one_label(side, side)


def stripes(h, w, n, along_rows):
    """n stripes of the labels 1 .. n: bands of rows (along_rows) or of columns"""
    if along_rows:
        lab = 1 + (np.arange(h) * n // h)[:, None] + np.zeros((1, w), dtype=np.int64)
    else:
        lab = 1 + (np.arange(w) * n // w)[None, :] + np.zeros((h, 1), dtype=np.int64)
    return u32(lab)


def stripes_depth2(h, w, n, along_rows):
    """the closed form for ``stripes``: every stripe is a rectangle"""
    out = np.zeros((h, w), dtype=np.uint32)
    edges = [int(np.searchsorted(np.arange(h if along_rows else w) * n // (h if along_rows else w), k)) for k in range(n + 1)]
    for k in range(n):
        (a, b) = (edges[k], edges[k + 1])
        if along_rows:
            out[a:b] = rectangle_depth2(b - a, w)
        else:
            out[:, a:b] = rectangle_depth2(h, b - a)
    return out


def disc(radius, inside=0, ring=0, margin=2):
    """a disc of label 1 (pixels with dy^2 + dx^2 <= radius^2) in a field of label ``inside``; ``ring`` > 0 cuts a
    concentric hole of that radius, of label ``inside``"""
    n = 2 * (radius + margin) + 1
    (y, x) = np.mgrid[0:n, 0:n] - (radius + margin)
    r2 = y * y + x * x
    seg = np.where((r2 <= radius * radius) & (r2 > ring * ring if ring else True), 1, inside)
    return u32(seg)


def ell(arm=HALO + 9, thick=2 * HALO + 5):
    """an L of label 1 in label 2: the pixels near its inner corner have their nearest foreign pixel diagonally"""
    n = arm + thick
    seg = np.full((n, n), 2, dtype=np.uint32)
    seg[:, :thick] = 1
    seg[arm:, :] = 1
    return seg


def u_shape(gap=5, thick=2 * HALO + 5):
    """a U of label 3 in label 0, its slot ``gap`` wide"""
    w = 2 * thick + gap
    seg = np.zeros((2 * thick + 4, w + 2), dtype=np.uint32)
    seg[1:-1, 1:-1] = 3
    seg[1:thick + 2, 1 + thick:1 + thick + gap] = 0
    return seg


def comb(teeth=6, tooth=7, gap=9, back=2 * HALO + 5, length=HALO + 2):
    """a comb of label 1 in label 2: a back ``back`` rows deep and teeth ``length`` long, ``tooth`` wide, ``gap`` apart"""
    w = teeth * tooth + (teeth - 1) * gap
    seg = np.full((back + length + 2, w + 2), 2, dtype=np.uint32)
    seg[1:1 + back, 1:-1] = 1
    for k in range(teeth):
        x0 = 1 + k * (tooth + gap)
        seg[1 + back:1 + back + length, x0:x0 + tooth] = 1
    return seg


def two_parts(side=2 * HALO + 3, gap=3):
    """label 5 in two squares of one size, the second below and right of the first: equal depth, the first is reported"""
    n = 2 * side + gap + 2
    seg = np.zeros((n, n), dtype=np.uint32)
    seg[1:1 + side, 1:1 + side] = 5
    seg[1 + side + gap:1 + 2 * side + gap, 1 + side + gap:1 + 2 * side + gap] = 5
    return seg


def pinhole(side=2 * HALO + 7):
    """a square of label 1 with a hole of label 0 one pixel wide near its middle, and a one-pixel slit"""
    seg = np.ones((side, side), dtype=np.uint32)
    seg[side // 2, side // 2 + 3] = 0
    seg[3:side // 3, side // 4] = 0
    return seg


def every_pixel_its_own(h=PH + 8, w=TW + 6):
    """h x w distinct labels: a patch holds PH x TW > SLOTS of them and takes the direct route"""
    return np.arange(1, h * w + 1, dtype=np.uint32).reshape(h, w)


def labels_in_patch(n, h=PH, w=TW):
    """one patch with exactly n distinct labels: n - 1 single pixels, the rest one label"""
    seg = np.full(h * w, n, dtype=np.uint32)
    seg[:n - 1] = np.arange(1, n, dtype=np.uint32)
    return seg.reshape(h, w)


def sparse_high_ids():
    """few labels, far apart in the id range"""
    seg = blocky((50, 90), 9, 5, 3, True).astype(np.int64)
    return u32(np.where(seg > 0, seg * 39989 + 11, 0))


SHAPES = {
    'disc_in_0_below_halo': lambda: disc(HALO - 2),
    'disc_in_0_at_halo': lambda: disc(HALO),
    'disc_in_2_above_halo': lambda: disc(HALO + 3, inside=2),
    'ring_in_0': lambda: disc(2 * HALO + 6, ring=5),
    'ring_in_2': lambda: disc(2 * HALO + 4, inside=2, ring=HALO // 2),
    'ell': ell,
    'u_shape': u_shape,
    'comb': comb,
    'two_parts': two_parts,
    'pinhole': pinhole,
}
# the shapes in which the window must defer pixels, and those in which it must not
SHAPES_DEFERRED = ('disc_in_2_above_halo', 'ell', 'u_shape', 'comb', 'two_parts')
SHAPES_NOT_DEFERRED = ('disc_in_0_below_halo',)


@functools.lru_cache(maxsize=None)
def shape(name):
    seg = SHAPES[name]()
    seg.setflags(write=False)
    return seg


EIGHT_CORES = (('core0', 0), ('core1', 1), ('core1h', 1.5), ('core2', 2), ('coreR8', 8 ** 0.5), ('core5', 5.0), ('coreHalo', HALO),
               ('coreMax', 32768))
